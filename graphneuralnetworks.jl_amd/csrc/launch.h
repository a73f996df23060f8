// launch.h — every host function that is called across translation units, declared ONCE, and the request structs those
// functions take.  The defining .hip and every caller include this header; a prototype is never copied into a .hip.
// (What common.h declares — fail, knob, the ensure_* plan helpers — stays there: those are the library's plumbing.)
// Sections: the row reduction, softmax_rows, the dense family, graph_chain2, column sums, plan.
#pragma once
#include "common.h"
#include "dense_route.h"

namespace gnnmp {

// ---- the row reduction (propagate.hip) --------------------------------------------------------------------------------------
// One call of csr_rows_kernel (+ its combine).  Fields are named after what they become in ReduceArgs (csr_reduce.h), where
// each one is documented; a call site sets only what it means.  A new optional input is a field here, a field in ReduceArgs
// and one line in run_reduce.
struct ReduceCall {
    const int32_t *idx = nullptr;   // per slot, the row of x to read: plan->col (propagate) or plan->eid (scatter)
    int aggr = GNNMP_SUM;
    const float *x = nullptr;
    const float *w = nullptr;
    const float *ss = nullptr;
    const float *w_slot = nullptr;
    const float *ss_slot = nullptr;
    const float *sd = nullptr;
    float *out = nullptr;
    int64_t D = 0;
    const float *emat = nullptr;
    const float *rowsub = nullptr;
    const float *gate_i = nullptr;
    int gated = 1;                  // the form gate_i selects (1 | 2); ignored without gate_i
    int act = 0;
    // reduce ONLY the split rows (their chunk virtual rows + the combine) and write row long_rows[r], finalised, to out[r] — a
    // compact [n_long][D] buffer the fused kernel reads instead of walking those rows (the caller sized the workspace and
    // passes out inside it)
    int long_only = 0;
    const float *bias = nullptr;
    int bias_relu = 0;
    const float *addend = nullptr;
    const float *mask_y = nullptr;
};
// shared by propagate (idx = col) and scatter (idx = eid)
int run_reduce(gnnmp_graph_t *p, const ReduceCall &c, hipStream_t stream);
// softmax over the rows of a plan, in the reference's three steps or the one-pass kernel of softmax_rows.hip
int run_softmax(gnnmp_graph_t *p, const float *e, float *alpha, int64_t D, float den_add, hipStream_t stream);
// fold plan->ws ([n_chunks][D] partials written by another kernel in the same virtual-row layout) into out's long rows;
// aggr: GNNMP_MAX, anything else sums
int run_combine(gnnmp_graph_t *p, float *out, int64_t D, int aggr, hipStream_t stream);

// ---- softmax_rows.hip ---------------------------------------------------------------------------------------------------------
// GNNMP_OK if it ran, 1 if the shape is not one it takes (the caller runs the three-step kernels)
int softmax_rows_try(gnnmp_graph_t *p, const float *e, float *alpha, int64_t D, float den_add, float *partial, float *mx, float *den,
                     hipStream_t stream);

// ---- the dense family (dense.hip, dense_split.hip, dense_wreg.hip, dense_t16.hip) ---------------------------------------
// gnnmp_dense_f32's arguments (gnnmp.h), validated.  dense_plan (dense_route.h) decides which kernel, which template instance and what
// launch geometry a call gets; gnnmp_dense_f32 keeps that DenseRoute in the calling thread's record (gnnmp_debug_dense_route) and calls
// the one launcher the route names.  A launcher maps the route's instance fields onto its template and fills the kernel's argument
// struct: it decides nothing, and a route that names no compiled instance is an error.
struct DenseCall {
    const float *x1, *W1;
    int64_t D1, ldw1;
    const float *x2, *W2;
    int64_t D2, ldw2;
    int w_layout;
    const float *bias;
    int act;
    float *out;
    int64_t N, Dout;
};
int dense_launch_split(const DenseCall &c, const DenseRoute &r, hipStream_t stream);    // dense_split.hip
int dense_launch_wreg(const DenseCall &c, const DenseRoute &r, hipStream_t stream);     // dense_wreg.hip
int dense_launch_t16(const DenseCall &c, const DenseRoute &r, hipStream_t stream);      // dense_t16.hip
int dense_launch_narrow(const DenseCall &c, const DenseRoute &r, hipStream_t stream);   // dense.hip
int dense_launch_wlds(const DenseCall &c, const DenseRoute &r, hipStream_t stream);     // dense.hip
int dense_launch_mfma(const DenseCall &c, const DenseRoute &r, hipStream_t stream);     // dense.hip
// element strides of W(j, k) at W[j * sj + k * sk]: w_layout 0 = W[Dout][K] (row j contiguous in k), 1 = W[K][Dout] (Julia column-major)
struct WStrides { int64_t sj, sk; };
inline WStrides w_strides(int w_layout, int64_t ldw) { return w_layout == 0 ? WStrides{ldw, 1} : WStrides{1, ldw}; }

// ---- graph_chain2.hip -----------------------------------------------------------------------------------------------------------
int graph_chain2_try(gnnmp_graph_t *p, const gnnmp_chain_jobs_t *J, const int64_t *seg_ptr, int64_t G, const float *x, int n_layers,
                     const int64_t *dims, const float *const *W_root, const float *const *W_agg, const float *const *bias,
                     const int *act, int w_layout, int aggr, int pool_aggr, const float *W_head, const float *b_head, int64_t nout,
                     float *out, hipStream_t stream);

// ---- column sums (dense_backward.hip) -----------------------------------------------------------------------------------------------
// Deterministic, two stages: every block of stage 1 sums one slab of rows, in row order, into part[slab][D]; the tree fold adds the
// slabs.  (The dense adjoints fold their slabs with fold_partials instead, in a different order: dense_backward.hip.)
int64_t colsum_slab_rows(int64_t N);   // rows a slab: at most 2048 slabs, of at least 256 rows
int colsum_parts(int64_t N);           // slabs of colsum_slab_rows(N) rows that cover N rows: what a workspace holds D floats for
// stage 1: part[b][d] = Σ_r x[r][d] (s null) or Σ_r s[r][d / C] * x[r][d] over the R rows of slab b < nparts; x [N][D], s [N][D / C]
int colsum_partial(const float *x, const float *s, int64_t N, int D, int C, int64_t R, int nparts, float *part, hipStream_t stream);
// the fold: out[(d / C) * out_ld + off + d % C] = Σ_p part[p][d] — thread k of 256 adds parts k, k + 256, ..., then a fixed tree
int colsum_tree_fold(const float *part, int nparts, int D, int C, int out_ld, int off, float *out, hipStream_t stream);

// ---- plan.hip -------------------------------------------------------------------------------------------------------------------
int plan_dispose(gnnmp_graph_t *p, hipStream_t stream, bool stream_known);
// GNNMP_OK if plan_t has plan's sizes transposed, GNNMP_EINVAL (message "<who>: ...", with the six sizes) otherwise
int check_transposed(const char *who, const gnnmp_graph_t *plan, const gnnmp_graph_t *plan_t);
// What the edge-level training exports ask of their plans, GNNMP_EINVAL with "<who>: ..." otherwise: the plan is square (need_square);
// plan_t, when given, has the plan's rows and edges; and — when the call has per-edge arrays, no_row saying which ("fs_e has no row for
// them") — the plan was not built with self loops of its own, which lie beyond those arrays' last row.
int check_edge_plan(const char *who, const gnnmp_graph_t *plan, const gnnmp_graph_t *plan_t, bool need_square, const char *no_row);

// ---- plan_batch.hip -------------------------------------------------------------------------------------------------------------
// A square plan of n_rows rows and n_slots slots whose rowptr / col / eid live in ONE block of the stream-ordered pool (pool.h), sizes,
// self-loop flag and long-row threshold set, index arrays not yet written: gnnmp_plan_select's allocation without a member table, for
// the plans plan_edit.hip derives.  The caller fills the arrays on `stream`, then sets max_degree / calls plan_build_long_rows.
int pooled_plan_alloc(gnnmp_graph_t **out, int64_t n_rows, int64_t n_slots, int self_loops, hipStream_t stream);

}  // namespace gnnmp
