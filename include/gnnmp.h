/*
 * gnnmp.h — C ABI of libgnnmp.so, the MI355X (gfx950) message-passing engine.
 *
 * This is the drop-in boundary for the GNNlib.jl hot path
 *   propagate / apply_edges / aggregate_neighbors  (GNNlib/src/msgpass.jl:71-79,121-129,145-149)
 * and the leaf ops it is built from
 *   _gather / _scatter                             (GNNGraphs/src/gatherscatter.jl:4,12-18)
 * The reference has no FFI: its device seam is the Julia package extension
 * GNNlib/ext/GNNlibAMDGPUExt.jl:13-32 (methods of GNNlib.propagate on AnyROCMatrix).  A replacement
 * extension `@ccall`s the symbols below (see INTEGRATION.md for the exact stub).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer, borrowed for the duration of the call only;
 *     the caller allocates inputs AND outputs.  The only long-lived object is the opaque plan.
 *   - feature arrays are Julia column-major (D, N)  ==  C row-major [N][D]: one node's / edge's
 *     feature vector is contiguous.  fp32 (every entry point) or fp64 (the *_f64 entry points: propagate, _gather, _scatter).
 *   - index arrays are passed exactly as the reference holds them: Int64 or Int32 (idx_bytes = 8 | 4),
 *     1-based (index_base = 1, Julia) or 0-based (index_base = 0).
 *   - `stream` is a hipStream_t (NULL = the null stream).  Compute entry points launch on it and
 *     return; they never call hipDeviceSynchronize and never allocate (exception: the first use of a
 *     plan with a row longer than GNNMP_LONG_ROW at a larger D than before grows plan-owned scratch
 *     with hipMalloc: the workspace of the split rows' partials and, since round 5, their slice
 *     partials and arrival counters — the split rows are folded inside the row kernels by the last
 *     chunk to arrive, not by a second launch).  gnnmp_plan_create synchronises `stream` (it is graph prep, done
 *     once per graph, outside the timed path).
 *   - stream capture (hipStreamBeginCapture / a HIP graph): a compute entry point may be recorded into a graph and replayed, with new
 *     values in the same buffers, any number of times back to back — ONE eager call with the same plan, entry point and D must come
 *     first (it grows the plan's scratch and opts the kernel into large LDS where it needs it; the exception above).  Not recordable:
 *     the calls whose comment says that they synchronise (plan builds and the other graph prep: gnnmp_batch_coo,
 *     gnnmp_sort_edge_index, gnnmp_unique_append, gnnmp_induced_subgraph, gnnmp_sample_neighbors, gnnmp_rand_edge_split,
 *     gnnmp_negative_sample, gnnmp_coalesce_edges, gnnmp_compact_edges, the host-result queries) and the arena.  What is TESTED (tests/test_abi_graph_capture.py, capture mode
 *     thread_local): every other export of the case table of tests/abi_cases.py — gnnmp_graphconv_chain_f32 among them, on both
 *     of its kernels and with host- and device-packed job handles, and once more through the Python mirror —
 *     gnnmp_hetero_propagate_f32 (tests/test_hetero.py) and gnnmp_hetero_propagate_grad_f32 (tests/test_hetero_backward.py) — those
 *     two without the eager call, they use no plan scratch — and gnnmp_edge_conv_f32 / gnnmp_edge_conv_grad_f32 (tests/test_edge_conv_ad.py)
 *     and gnnmp_cg_conv_grad_f32 (tests/test_cg_conv_ad.py) and gnnmp_nn_conv_grad_f32 (tests/test_nn_conv_ad.py) and gnnmp_egnn_edge_f32 /
 *     gnnmp_egnn_coord_f32 / gnnmp_egnn_coord_grad_f32 / gnnmp_act_grad_z_f32 (tests/test_egnn_conv_ad.py) and gnnmp_gmm_conv_f32 / gnnmp_gmm_conv_grad_f32 /
 *     gnnmp_gmm_weights_grad_f32 (tests/test_gmm_conv_ad.py) and gnnmp_megnet_edge_f32 / gnnmp_megnet_edge_grad_f32 /
 *     gnnmp_aggregate_grad_f32 (tests/test_megnet_conv_ad.py) and gnnmp_segment_attn_pool_f32 / gnnmp_segment_attn_pool_grad_f32 /
 *     gnnmp_lstm_pointwise_grad_f32 (tests/test_readout_ad.py) and
 *     gnnmp_poly_hop_f32 (tests/test_poly_conv_ad.py: over the plan and the transposed plan) and
 *     gnnmp_gru_pointwise_grad_f32 (tests/test_poly_conv_ad.py) and gnnmp_poly_hop_ld_f32 / gnnmp_gru_cell_f32 / gnnmp_gru_cell_grad_f32 /
 *     gnnmp_lstm_cell_f32 / gnnmp_lstm_cell_grad_f32 (tests/test_recurrent_layers.py) and gnnmp_lstm_matvec_cell_f32 /
 *     gnnmp_lstm_matvec_grad_f32 / gnnmp_outer_accum_f32 (tests/test_evolve_gcno.py: a whole training step) and
 *     gnnmp_attn_conv_edge_f32 / gnnmp_attn_conv_edge_grad_f32 (tests/test_attn_edge.py), likewise.  Not tested and not promised: the lifecycle calls — gnnmp_plan_concat / gnnmp_plan_select / gnnmp_chain_jobs_pack make
 *     no host synchronisation when the pool holds a stream-released block that fits (a warm pool), but a miss is a hipMalloc and a
 *     block parked by a plain destroy costs a device synchronisation: create such objects outside a capture.
 *   - a plan carries scratch of its own (the partials of split rows, the tile ticket of the fused layer kernel, cached
 *     orderings): calls that take the SAME plan must be ordered on ONE stream (or by events) — two streams may run
 *     different plans, or read-only queries of one plan, concurrently, but not two compute calls on one plan.  The
 *     reference has the same shape: one GNNGraph, one task.  Host threads: besides the tuning knobs (gnnmp_tune, experiments
 *     only) and the thread-local error string, the library's only process-wide state is (i) the per-DEVICE tables behind a mutex —
 *     which kernels have been opted into large LDS on which device, and the stream-ordered block pool that backs
 *     gnnmp_plan_concat / gnnmp_plan_select / gnnmp_chain_jobs_pack (one table per device: a block, its event and its stream are
 *     only ever matched against takers of the SAME device) — and (ii) a per-thread scratch cache of graph prep, keyed on the device.
 *   - several devices in one process (a Julia host calling AMDGPU.device!(d) between calls): supported.  Every entry point acts on
 *     the calling thread's CURRENT device (hipGetDevice) — the one `stream` and every pointer of the call must belong to.  Plans,
 *     job handles and arenas belong to the device they were created on; gnnmp_arena_* refuse a foreign current device with
 *     GNNMP_EINVAL.  Release a pooled object (gnnmp_plan_release, gnnmp_chain_jobs_release) with a stream of ITS device.
 *   - return value: 0 = ok, negative = gnnmp_status; nothing throws, nothing aborts.
 *     gnnmp_last_error() gives a thread-local message for the last failing call.
 *   - determinism: no entry point except *_atomic_* uses floating-point atomics.  Per-destination
 *     reductions run in the ORIGINAL COO edge order (the order NNlib.scatter uses on the CPU) for
 *     rows of at most GNNMP_LONG_ROW edges — bit-identical to the reference CPU gather->scatter
 *     path; longer rows are split into fixed chunks combined in fixed order (run-to-run
 *     deterministic, within 1e-5 rel of the sequential sum).
 */
#ifndef GNNMP_H
#define GNNMP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GNNMP_VERSION 100 /* 0.1.0 */

typedef void *gnnmp_stream_t;           /* hipStream_t */
typedef struct gnnmp_graph gnnmp_graph_t; /* opaque: dst-sorted CSR plan of one (s, t) edge index */

typedef enum {
    GNNMP_OK = 0,
    GNNMP_EINVAL = -1,       /* bad argument (null pointer, bad enum, bad size)            */
    GNNMP_EBOUNDS = -2,      /* index outside 1..N (validate != 0 only)                    */
    GNNMP_EALLOC = -3,       /* hipMalloc failed                                           */
    GNNMP_ELAUNCH = -4,      /* kernel launch / HIP runtime error                          */
    GNNMP_EUNSUPPORTED = -5  /* valid request outside the build's envelope (e.g. E' >= 2^32 - 65536) */
} gnnmp_status;

/* aggregation operator — the `aggr` argument of propagate / aggregate_neighbors / reduce_nodes
 * (GNNGraphs/src/gatherscatter.jl:12-18 -> NNlib.scatter).  Empty destinations keep the identity:
 * 0 for SUM and MEAN, -Inf for MAX, +Inf for MIN.  MEAN = sum / count (true division). */
typedef enum { GNNMP_SUM = 0, GNNMP_MEAN = 1, GNNMP_MAX = 2, GNNMP_MIN = 3 } gnnmp_aggr;

/* built-in message functions with a fused path (GNNlib/src/msgpass.jl:162,191-208).
 * E_MUL_XJ with a vector `e` is W_MUL_XJ with w = e (msgpass.jl:223-228). */
typedef enum { GNNMP_COPY_XJ = 0, GNNMP_W_MUL_XJ = 1 } gnnmp_msg;

/* activation fused into gnnmp_dense_f32's epilogue (the layers' `σ`): IDENTITY and RELU everywhere an `act` is taken;
 * SOFTPLUS (NNlib.softplus = log1p(exp(-|x|)) + relu(x)) and TANH also as the second factor of gnnmp_propagate_cg_f32 and
 * in gnnmp_bias_act_f32; SWISH (x * sigmoid(x), egnn_conv's Dense layers) in gnnmp_bias_act_f32, gnnmp_egnn_edge_f32 and
 * gnnmp_act_grad_z_f32 only. */
typedef enum {
    GNNMP_ACT_IDENTITY = 0, GNNMP_ACT_RELU = 1, GNNMP_ACT_SOFTPLUS = 2, GNNMP_ACT_TANH = 3, GNNMP_ACT_SWISH = 4
} gnnmp_act;
/* per-edge attention logit of gnnmp_attn_conv_f32 (Q_i = row i of the target array, K_j = row j of the source array) */
typedef enum {
    GNNMP_ATTN_GAT = 0,   /* leakyrelu(a[h][0:C] . Q_i + a[h][C:2C] . K_j)      gat_message   conv.jl:152-167 */
    GNNMP_ATTN_GATV2 = 1, /* a[h] . leakyrelu(Q_i + K_j)                        gatv2_message conv.jl:202-214 */
    GNNMP_ATTN_DOT = 2,   /* (Q_i . K_j) / scale, values from a third array     transformer_message_uij conv.jl:609-616 */
    GNNMP_ATTN_COS = 3    /* scale * cos(Q_i, K_j), single head                 agnn_conv     conv.jl:337-352 */
} gnnmp_attn;

/* Destinations with more edges than the plan's threshold are split into balanced chunks (see determinism note
 * above).  The threshold is chosen per plan in [GNNMP_MIN_LONG_ROW, GNNMP_LONG_ROW] from the graph size
 * (~4e-5 * E', so that no single sequential row can become the kernel's tail) and reported by gnnmp_plan_info
 * (info[7]); rows of at most GNNMP_MIN_LONG_ROW edges are never split. */
#define GNNMP_LONG_ROW 512
/* a plan holds fewer than this many slots (edges + added self loops): slots and edge positions are unsigned 32-bit values, with
 * headroom so that no slot counter inside a kernel can wrap */
#define GNNMP_MAX_SLOTS 4294901760LL /* 2^32 - 65536 */
#define GNNMP_MIN_LONG_ROW 64

int gnnmp_version(void);
const char *gnnmp_last_error(void);

/* ------------------------------------------------------------------------------------------------
 * Plan: the graph side of GNNGraph{COO_T} (GNNGraphs/src/gnngraph.jl:108-117) as the kernels want it.
 * Built once per (s, t) pair; replaces the per-call `sparse(s,t,...)` rebuild of the reference fast path
 * (GNNlib/src/msgpass.jl:215-218 -> GNNGraphs/src/convert.jl:221-237) and the per-call index
 * concatenation of add_self_loops (GNNGraphs/src/transform.jl:12-28).
 *
 *   src, dst     : s and t, n_edges entries each (edge k goes src[k] -> dst[k]).
 *   n_src, n_dst : number of source / destination nodes (equal for GNNGraph; different for the bipartite
 *                  case of GNNlib/src/utils.jl:123-125 and for reduce_nodes-as-scatter).
 *   add_self_loops != 0 : append the edges (i, i), i = 1..n (requires n_src == n_dst), AFTER the given
 *                  edges, exactly like transform.jl:12-28 (never de-duplicates).  E' = n_edges + n.
 *   validate != 0: check 1 <= s <= n_src, 1 <= t <= n_dst on the device (GNNGraphs/src/convert.jl:47-54)
 *                  and return GNNMP_EBOUNDS instead of building.
 * The plan stores: rowptr[n_dst+1] (unsigned 32-bit), col[E'] (0-based source of each slot, int32), eid[E'] (0-based original
 * edge position of each slot, unsigned 32-bit; self loops are n_edges + i).  Slots of one destination keep the original
 * edge order (stable sort).  Limits: n_src, n_dst < 2^31 - 1 and E' < GNNMP_MAX_SLOTS = 2^32 - 65536 (COO_T admits any
 * Integer, GNNGraphs/src/abstracttypes.jl:1: the INDEX type may be Int64 at any size; the COUNT of edges of one plan is
 * bounded by the 32-bit slots); beyond that GNNMP_EUNSUPPORTED.
 * ---------------------------------------------------------------------------------------------- */
int gnnmp_plan_create(gnnmp_graph_t **out, const void *src, const void *dst, int idx_bytes,
                      int index_base, int64_t n_src, int64_t n_dst, int64_t n_edges,
                      int add_self_loops, int validate, gnnmp_stream_t stream);
/* The plan of a GNNGraph{SPARSE_T} (GNNGraphs/src/abstracttypes.jl:5, gnngraph.jl:108): the graph IS a compressed-sparse-column
 * adjacency A with A[s, t] != 0 for an edge s -> t, and the reference's device seam takes such graphs next to COO ones
 * (GNNlib/ext/GNNlibAMDGPUExt.jl:13-32 dispatches on Union{COO_T, SPARSE_T}).  Column t of A lists the sources of t's incoming edges
 * in ascending order, and edge_index(g) = findnz(A) walks the columns in order (GNNGraphs/src/query.jl:14, convert.jl:62-73): the
 * edges of a sparse graph are ALREADY destination-sorted and the plan is the CSC structure itself — no sort:
 *      rowptr = colptr - index_base      col = rowval - index_base      eid[p] = p   (edge k of edge_index(g) is slot k)
 * so that edge data in findnz order (get_edge_weight(g) = nzval, query.jl:18) is what `w` / `e` of the propagate entry points take.
 *   colptr : n_dst + 1 column pointers (SparseMatrixCSC.colptr / ROCSparseMatrixCSC.colPtr), rowval : n_edges row indices.
 *   colptr[1] = 1, colptr[end] = n_edges + 1, non-decreasing, 1 <= rowval <= n_src are ALWAYS checked on the device (GNNMP_EBOUNDS) —
 *   the build synchronises the stream anyway; `validate` is accepted for symmetry with gnnmp_plan_create and ignored.
 * Stored entries whose VALUE is zero are edges: a sparse graph's num_edges is nnz(A) (convert.jl:199) and its edge_index is
 * to_coo(A::SPARSE_T) = findnz(A) (convert.jl:62-73), which walks the STORED entries, explicit zeros included — the `findall(!=(0), A)` of
 * convert.jl:75-79 is the dense-matrix method.  Same limits and the same stream synchronisation as gnnmp_plan_create. */
int gnnmp_plan_from_csc(gnnmp_graph_t **out, const void *colptr, const void *rowval, int idx_bytes, int index_base, int64_t n_src,
                        int64_t n_dst, int64_t n_edges, int validate, gnnmp_stream_t stream);
int gnnmp_plan_destroy(gnnmp_graph_t *plan);
/* info[0]=n_src info[1]=n_dst info[2]=n_edges (as given) info[3]=E' (with self loops)
 * info[4]=max in-degree info[5]=number of split (long) rows info[6]=bytes of device memory held */
int gnnmp_plan_info(const gnnmp_graph_t *plan, int64_t info[8]);
/* copy the plan's index arrays into caller device buffers (any may be NULL): int32 rowptr[n_dst+1],
 * col[E'], eid[E'] — bit-exact index outputs, used by the parity tests.  GNNMP_EUNSUPPORTED when E' >= 2^31 (the values do
 * not fit int32): gnnmp_plan_export64 hands out rowptr widened to int64 and eid as the unsigned values they are, at any size. */
int gnnmp_plan_export(const gnnmp_graph_t *plan, int32_t *rowptr, int32_t *col, int32_t *eid,
                      gnnmp_stream_t stream);
int gnnmp_plan_export64(const gnnmp_graph_t *plan, int64_t *rowptr, int32_t *col, uint32_t *eid,
                        gnnmp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * The plan of a BATCH without a sort (csrc/plan_batch.hip).  MLUtils.batch(gs) (GNNGraphs/src/transform.jl:682-709) offsets the
 * members' node ids by the nodes before them and concatenates their edge lists member after member, so the batch's dst-sorted stable
 * CSR is the concatenation of the members' CSRs (rowptr pieces shifted by the slots before them, col by the nodes, edge positions by the
 * edges; plan-added self loops stay at E_batch + node).  The reference's graph-classification loop makes a new batch EVERY step
 * (GraphNeuralNetworks/examples/graph_classification_tudataset.jl:70-71 DataLoader(...; shuffle = true, collate = true), :97-104): these
 * entry points are per-step work — two launches, NO host synchronisation, index arrays from a stream-ordered pool of device blocks — and
 * the result is bit-identical to gnnmp_plan_create on the batched COO (tests/test_plan_batch.py).
 *
 *   gnnmp_plan_concat  members as plan handles, in batch order (what a `batch(gs)` override holds: one cached plan per member graph;
 *                      all square, all with or all without added self loops).  The member table (48 bytes per member) is built on the
 *                      host and uploaded with the call.
 *   gnnmp_plan_select  members as graph ids (ids[k], idx_bytes / index_base like every index array) into ONE resident plan of the whole
 *                      dataset batched once — `dataset` = the plan of MLUtils.batch(all graphs), node_ptr[n_graphs + 1] (device, int64)
 *                      its node offsets — in the order of `ids`: the plan of batch(gs[ids]), which is also what getobs / getgraph of a
 *                      batched graph returns for ascending ids (GNNGraphs/src/gnngraph.jl:311, transform.jl:827-876).  Nothing crosses
 *                      PCIe per step.  The dataset's edge list must be member-major (what batch produces).  n_rows / n_slots: the
 *                      batch's node count and its E' (edges + added self loops if the dataset plan has them), which the caller knows
 *                      on the host (every GNNGraph carries num_nodes / num_edges as host integers); they size the allocation.  If they
 *                      disagree with the selected members the plan comes out EMPTY (rowptr = 0) and gnnmp_plan_status reports it.
 *   Optional outputs (device, NULL to skip): seg_ptr_out int64[k + 1] the batch's node offsets (the seg_ptr of gnnmp_graphconv_chain_f32
 *   / gnnmp_segment_pool_ptr_f32), node_map_out int32[n_rows] the dataset row of every batch row (0-based: the `nmap` of getgraph; feed
 *   it to gnnmp_gather_f32 to collate node features), graph_indicator_out [n_rows] in the index type of `ids` (concat: idx_bytes /
 *   index_base arguments).
 * Rows longer than the new plan's long-row threshold (hubs) need the chunk tables: only then the call synchronises the stream.
 * gnnmp_plan_info's max in-degree of a selected plan is the dataset's (an upper bound).
 *
 *   gnnmp_plan_release  stream-ordered destroy: the plan's block returns to the pool behind the work enqueued on `stream` so far; the next
 *                      pooled object created on ANY stream waits for that work on the device (no host synchronisation).  The caller
 *                      promises that no later work uses the plan.  gnnmp_plan_destroy works on these plans too (the block is then handed
 *                      out again only after a device-wide synchronisation).
 *   gnnmp_plan_edge_index  s, t of the plan's graph in original edge order (plan-added self loops skipped): the batch's COO for callers
 *                      that want it (out_src / out_dst: n_edges entries of idx_bytes each).
 * ---------------------------------------------------------------------------------------------- */
int gnnmp_plan_concat(gnnmp_graph_t **out, const gnnmp_graph_t *const *members, int64_t k, int64_t *seg_ptr_out,
                      void *graph_indicator_out, int idx_bytes, int index_base, gnnmp_stream_t stream);
int gnnmp_plan_select(gnnmp_graph_t **out, const gnnmp_graph_t *dataset, const int64_t *node_ptr, int64_t n_graphs, const void *ids,
                      int idx_bytes, int index_base, int64_t k, int64_t n_rows, int64_t n_slots, int64_t *seg_ptr_out,
                      int32_t *node_map_out, void *graph_indicator_out, gnnmp_stream_t stream);
int gnnmp_plan_release(gnnmp_graph_t *plan, gnnmp_stream_t stream);
int gnnmp_plan_status(const gnnmp_graph_t *plan, gnnmp_stream_t stream);   /* synchronises `stream`; 0 = the member table matched */
int gnnmp_plan_edge_index(const gnnmp_graph_t *plan, int idx_bytes, int index_base, void *out_src, void *out_dst,
                          gnnmp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * The plan of an EDITED graph from the plan of its parent, without a sort of the parent's edges (csrc/plan_edit.hip): the structural
 * augmentations remove_nodes, add_edges, add_nodes and perturb_edges (GNNGraphs/src/transform.jl:212-276, 319-353, 385-420, 553-561) are
 * applied to a fresh batch on every training step, and the child's dst-sorted stable CSR is a filtered, relabelled copy of the parent's:
 * dropping nodes keeps the surviving slots of every surviving row in their order, appending edges only adds slots at the end of rows.
 * Both results are bit-identical to gnnmp_plan_create on the child's COO with the parent's self-loop flag (rowptr, col, eid, and
 * gnnmp_plan_info except the bytes held; tests/test_plan_edit.py), live in ONE block of the stream-ordered pool like the plans of
 * gnnmp_plan_select (gnnmp_plan_release / gnnmp_plan_destroy both work on them), and leave the parent untouched.  `parent` must be square
 * (n_src == n_dst = N), with or without plan-added self loops.  Only square-ness is assumed: the same call on the parent's TRANSPOSED plan
 * (add_edges: with s_new and t_new swapped) gives the child's transposed plan with the same edge numbering.  gnnmp_plan_edge_index gives
 * the child's s, t.
 *
 *   gnnmp_plan_remove_nodes  the plan of remove_nodes(g, nodes) / remove_nodes(g, p).
 *       remove != NULL (list mode): n_remove node ids (idx_bytes / index_base like every index array), in any order, repeats allowed (the
 *                      reference's sort(union(...)) allows them); p must be 0.  An id outside index_base .. N - 1 + index_base gives
 *                      GNNMP_EBOUNDS — the reference does not check this (such an id only lowers its num_nodes).
 *       remove == NULL (random mode): node i is removed exactly when gnnmp_dropout_keep_u8(seed, p, N, 1) would write keep[i][0] == 0
 *                      (0 <= p <= 1; p = 1 removes every node) — a pure function of (seed, i), not Julia's RNG stream.
 *       The kept nodes keep their ascending order and are renumbered 0 .. n_keep - 1; an edge survives iff both its endpoints do, and the
 *       surviving edges keep their relative order and are renumbered 0 .. E_keep - 1 by their rank in the parent's edge list; a plan-added
 *       self loop of a kept node stays, at E_keep + its new id.
 *       Optional outputs (device, NULL to skip): node_map_out int32[n_keep] the old 0-based id of every child node (ascending);
 *       node_new_out int32[N] the new 0-based id of every parent node, -1 for a removed one (written whole); edge_map_out uint32[E_keep]
 *       the old 0-based position of every child edge (ascending).  The caller sizes node_map_out / edge_map_out for the worst case (N, E)
 *       or from a first call; only the first n_keep / E_keep entries are written.
 *       total (HOST memory, int64[2], required): total[0] = n_keep, total[1] = E_keep, always written.
 *       ONE host synchronisation of `stream` (the two totals size the allocation); a second one only when a row of the child is longer than
 *       the child's own long-row threshold (the chunk tables, as in every plan build).  Five integer passes (mark, scan, per-slot keep +
 *       scans, fill); no float work, no sort.
 *
 *   gnnmp_plan_add_edges  the plan of add_edges(g, s_new, t_new) on n_nodes >= N nodes (nodes N .. n_nodes - 1 are new and isolated: with
 *       m = 0 this is add_nodes), E + m edges: the parent's at their positions, the new ones at E .. E + m - 1.
 *       s_new, t_new != NULL (list mode): m new edges; indices outside index_base .. n_nodes - 1 + index_base give GNNMP_EBOUNDS (checked
 *                      on the device before anything is built).  s_new_out / t_new_out are ignored.
 *       s_new == t_new == NULL (random mode, perturb_edges): new edge k is the ordered pair  s = mulhi32(h(k, 0), N),
 *                      t' = mulhi32(h(k, 1), N - 1), t = t' + (t' >= s)  with h(k, j) the 32 bits gnnmp_dropout_keep_u8's hash gives for
 *                      (seed, e = k, head = j) and mulhi32(a, b) = (a * b) >> 32 — uniform over the ordered pairs of the PARENT's nodes with
 *                      s != t, the distribution of the reference's rejection loop, reproducible on the host.  The pairs are written to
 *                      s_new_out / t_new_out (required; m entries of idx_bytes each, in index_base).  N < 2 with m > 0 is GNNMP_EINVAL (the
 *                      reference's assertion).
 *       Every row of the child is the parent's row followed by its new slots in position order; plan-added self loops are renumbered to
 *       E + m + node and new nodes get theirs.
 *       EVERY mode synchronises `stream`: the m new edges are grouped by destination with the stable radix sort (on them only, never on the
 *       parent's E), and the chunk-table pass reads the child's longest row back, as gnnmp_plan_create does.  There is no
 *       synchronisation-free path.
 *
 *   gnnmp_plan_keep_nodes  gnnmp_plan_remove_nodes with the mask SUPPLIED instead of marked (TopKPool — GNNlib/src/layers/pool.jl:14-27: the
 *       child of view(A, idx, idx)): node i stays iff keep[i] != 0.  keep is a device array uint32[N] — what gnnmp_topk_select_f32 wrote
 *       (its closing word keep[N] is not read).  Everything after the mark is the same code as gnnmp_plan_remove_nodes: the same child, the
 *       same optional outputs and totals, ONE host synchronisation of `stream` (a second one for a child with a long row).  keep == NULL is
 *       GNNMP_EINVAL unless N = 0.
 *
 *   Refusals (before any device work): out / parent / total NULL, a non-square parent, idx_bytes / index_base, p outside [0, 1] (or p != 0
 *   in list mode), negative counts, n_nodes < N, one of s_new / t_new alone, a NULL random-mode output: GNNMP_EINVAL; a child of
 *   GNNMP_MAX_SLOTS slots or more (or 2^31 - 1 nodes): GNNMP_EUNSUPPORTED.
 * ---------------------------------------------------------------------------------------------- */
int gnnmp_plan_remove_nodes(gnnmp_graph_t **out, const gnnmp_graph_t *parent, const void *remove, int idx_bytes, int index_base,
                            int64_t n_remove, float p, uint64_t seed, int32_t *node_map_out, int32_t *node_new_out,
                            uint32_t *edge_map_out, int64_t *total, gnnmp_stream_t stream);
int gnnmp_plan_add_edges(gnnmp_graph_t **out, const gnnmp_graph_t *parent, const void *s_new, const void *t_new, int idx_bytes,
                         int index_base, int64_t m, int64_t n_nodes, uint64_t seed, void *s_new_out, void *t_new_out,
                         gnnmp_stream_t stream);
int gnnmp_plan_keep_nodes(gnnmp_graph_t **out, const gnnmp_graph_t *parent, const uint32_t *keep, int32_t *node_map_out,
                          int32_t *node_new_out, uint32_t *edge_map_out, int64_t *total, gnnmp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * A placement-aware arena for the OUTPUTS of the gather kernels (csrc/arena.hip) — optional: the rule "the caller allocates" stands,
 * this is an allocator the caller may use.  Measured on MI355X (profiles/README.md, round 4): device memory falls into three placement
 * classes of 96 GiB of physical HBM each; a kernel that gathers ~27 random rows per row it writes (propagate, the fused GCN layer, the
 * one-pass attention) runs 6 % slower when the gathered matrix and the output lie in the SAME class than when they lie in two — and
 * hipMalloc pairs buffers by luck.  The arena allocates 2 GiB blocks one by one (plain hipMalloc), classifies each where it lies with a
 * 0.6 ms probe (a propagate over a synthetic random graph, timed with the block as its output at four places: 10 % apart between the two
 * cases) and keeps blocks of n_classes = 2 or 3 different classes (three let a pipeline keep the PREVIOUS kernel's output — whose dirty
 * lines are still being written back — out of the class the next kernel gathers from); the other blocks are freed:
 *   gnnmp_arena_create(&a, bytes_per_class, n_classes, max_probe_bytes, stream)   bytes_per_class rounded up to 2 GiB blocks.  Creation works
 *                        inside a BUDGET: at most max_probe_bytes (<= 0: 32 GiB) of blocks held at any moment while the classes are being
 *                        looked for (they come in runs of GiB to tens of GiB) and ~0.3 s (env GNNMP_ARENA_BUDGET_MS); a block is screened at
 *                        one window, the kept ones checked at four.  Out of budget is NOT an error: the arena comes back with the classes
 *                        it found — info[7] = 0 .. n_classes of them, info[9] = 1 — and the caller places what it can (two classes still
 *                        separate a gather's source from its output; fewer: allocate as usual).  Synchronises.
 *   gnnmp_arena_class_of(a, ptr, bytes, &cls, stream)   arena memory: its range (0 .. classes - 1), no launch.  Foreign memory (bytes >= 128 MiB):
 *                        the probe with `ptr` as the gathered matrix and the output in every range — c = it shares range c's class,
 *                        classes = none of them / mixed / too small to tell / no room left for the probe's output; synchronises
 *   gnnmp_arena_alloc(a, cls, bytes, &ptr)   bump allocation (4 KiB aligned) inside one block of class cls; a buffer LARGER than a block
 *                        (SAGEConv's 2.5 GB output on the products shape) is an allocation of its own, classified where it lies when it
 *                        is asked for (every 512 MiB window probed, all must agree; up to three tries; SYNCHRONISES THE DEVICE and holds the
 *                        arena's lock meanwhile — set-up work for a persistent buffer, tens of milliseconds: the arena is NOT a compute
 *                        entry point and the "never synchronise" rule above does not cover it; a layer that asks for a placed output pays
 *                        this on its first call only.  At most one unused buffer of another class is retained as a spare, the other
 *                        misses are freed before the call returns); GNNMP_EALLOC when the class cannot serve it (the caller then
 *                        allocates as usual)
 *   gnnmp_arena_reset(a)  forget every allocation (the caller knows nothing uses them any more)
 *   gnnmp_arena_info      info[14]: [0] bytes per class asked for [1], [2], [8] bytes used in range 0 / 1 / 2 [3] blocks created while classifying
 *                         [4] released again [5], [6] the probe's microseconds with source and output in one class / in two [7] classes held
 *                         [9] 1 = gave up on the budget [10], [11], [12] blocks held per range [13] microseconds creation took
 * ALIASING: the arena is a bump allocator — memory it hands out stays handed out until gnnmp_arena_reset.  A caller that keeps a layer's
 * output buffer in the arena and passes the SAME buffer to the layer's next call (gnnmp/placement.py's persistent outputs, the static
 * outputs of a captured graph) overwrites the previous result; a caller that needs both alive allocates both.
 * Usage: cls = class_of(gathered matrix); out = alloc(any range != cls).  Results do not depend on where buffers lie.
 * ---------------------------------------------------------------------------------------------- */
typedef struct gnnmp_arena gnnmp_arena_t;
int gnnmp_arena_create(gnnmp_arena_t **out, int64_t bytes_per_class, int n_classes, int64_t max_probe_bytes, gnnmp_stream_t stream);
int gnnmp_arena_destroy(gnnmp_arena_t *arena);
int gnnmp_arena_alloc(gnnmp_arena_t *arena, int cls, int64_t bytes, void **ptr);
int gnnmp_arena_reset(gnnmp_arena_t *arena);
int gnnmp_arena_class_of(gnnmp_arena_t *arena, const void *ptr, int64_t bytes, int *cls, gnnmp_stream_t stream);
int gnnmp_arena_info(const gnnmp_arena_t *arena, int64_t *info);

/* ------------------------------------------------------------------------------------------------
 * Index ops (bit-exact)
 * ---------------------------------------------------------------------------------------------- */
/* add_self_loops(g::GNNGraph{COO}) — GNNGraphs/src/transform.jl:12-28.
 * out_src/out_dst have n_edges + n entries of the same width/base as the inputs; w / out_w may both be
 * NULL (unweighted) or both non-NULL (appended weights are 1). */
int gnnmp_add_self_loops(const void *src, const void *dst, int idx_bytes, int index_base,
                         int64_t n_edges, int64_t n, void *out_src, void *out_dst, const float *w,
                         float *out_w, gnnmp_stream_t stream);

/* MLUtils.batch(::Vector{GNNGraph{COO}}) index part — GNNGraphs/src/transform.jl:682-709.
 * src/dst hold the member graphs' edge indices concatenated (local numbering); edge_ptr[G+1] and
 * node_ptr[G+1] are int64 device arrays of exclusive prefix sums of num_edges / num_nodes.
 * Writes the offset indices (same width/base) and graph_indicator[N] (same width; values
 * index_base .. index_base+G-1, i.e. 1..G for Julia).
 * Synchronises the stream (graph prep: the two totals are read on the host). */
int gnnmp_batch_coo(const void *src, const void *dst, int idx_bytes, int index_base,
                    const int64_t *edge_ptr, const int64_t *node_ptr, int64_t n_graphs,
                    void *out_src, void *out_dst, void *graph_indicator, gnnmp_stream_t stream);

/* sort_edge_index(u, v) — GNNGraphs/src/utils.jl:30-45: the pairs (u_k, v_k) sorted lexicographically (by u, then v),
 * one common permutation.  64-bit radix sort of the packed pairs on the device (the reference's CUDA extension copies
 * the index to the CPU for this, GNNGraphsCUDAExt.jl:24-30).  Indices must fit 32 bits (GNNMP_EBOUNDS otherwise).
 * Synchronises the stream (graph prep). */
int gnnmp_sort_edge_index(const void *u, const void *v, int idx_bytes, int index_base, int64_t n_edges,
                          void *u_out, void *v_out, gnnmp_stream_t stream);
/* is_bidirected(g) — GNNGraphs/src/query.jl:553-558: sort_edge_index(s, t) == sort_edge_index(t, s); *result = 0 | 1 (host). */
int gnnmp_is_bidirected(const void *s, const void *t, int idx_bytes, int index_base, int64_t n_edges,
                        int *result, gnnmp_stream_t stream);
/* has_self_loops(g) — GNNGraphs/src/query.jl:565-569: any(s .== t); *result = 0 | 1 (host). */
int gnnmp_has_self_loops(const void *s, const void *t, int idx_bytes, int64_t n_edges, int *result,
                         gnnmp_stream_t stream);
/* The edge selection of sample_neighbors(g, nodes, K; dir, replace) — GNNGraphs/src/sampling.jl:68-83.  For seed i
 * (nodes[i], in the plan's destination numbering) with d incoming edges, draws k_i = (K > 0 ? (replace ? K : min(d, K))
 * : d) of them (0 if d = 0): without replacement every k-subset is equally likely (selection sampling; the chosen edges
 * keep their original order), with replacement k independent uniform picks (replace = 2: min(d, K) picks with
 * replacement, what NeighborLoader's `rand(neighbors, min(K, d))` draws, samplers.jl:56-62).  dir = :in uses the graph's plan, dir = :out
 * a plan of the reversed edge index.  Outputs: offsets[n_nodes + 1] (device, int64, exclusive prefix sums of k_i),
 * eids_out[offsets[n_nodes]] = original edge positions (index width / base of `nodes`), *total (host).  capacity =
 * entries available in eids_out; if too small GNNMP_EINVAL is returned with *total and offsets valid.  The generator is
 * counter based (seed, seed-node position, draw index): the same call returns the same sample; it is NOT Julia's RNG
 * stream, so parity with the reference is distributional (tests check membership, counts, uniqueness, uniformity).
 * Synchronises the stream. */
int gnnmp_sample_neighbors(gnnmp_graph_t *plan, const void *nodes, int idx_bytes, int index_base, int64_t n_nodes,
                           int64_t K, int replace, uint64_t seed, int64_t *offsets, void *eids_out,
                           int64_t capacity, int64_t *total, gnnmp_stream_t stream);

/* Ordered node sets on the device (the `Set` / `Dict(node => i)` bookkeeping of NeighborLoader, samplers.jl:78-99, and of
 * induced_subgraph, sampling.jl:178).  map[n_nodes] (int32, zero-initialised by the caller) holds 0 for "absent" and the
 * 1-based list position otherwise; first[n_nodes] is int32 scratch.  Appends to the set the candidates that are not in
 * it yet, each once, in order of first occurrence: writes them to list_out[0 .. *n_new) (index width / base of `cand`)
 * and map[v] = set_size + position + 1.  Deterministic (no dependence on thread scheduling).  Synchronises the stream. */
int gnnmp_unique_append(int32_t *map, int32_t *first, int64_t n_nodes, const void *cand, int idx_bytes,
                        int index_base, int64_t n_cand, int64_t set_size, void *list_out, int64_t *n_new,
                        gnnmp_stream_t stream);
/* induced_subgraph(graph, nodes) — GNNGraphs/src/sampling.jl:173-203: for every listed node i (in list order) its incoming
 * edges (in edge order) whose source is listed too, relabelled by list position: s_out = map[source], t_out = position of
 * i, eid_out = the edge's position in g.  `map` as built by gnnmp_unique_append from the same list (nodes must be valid
 * and distinct).  offsets[n_nodes + 1] (device int64) = first output edge of every listed node; *total (host) = edge
 * count; capacity as in gnnmp_sample_neighbors (capacity = 0 with NULL outputs = count-only call).  NB the reference records `findfirst` of the (source, target) pair as the
 * edge index, i.e. the FIRST parallel edge for all copies of a multi-edge; this returns each copy's own position.
 * Synchronises the stream (the count is read on the host). */
int gnnmp_induced_subgraph(gnnmp_graph_t *plan, const int32_t *map, const void *nodes, int idx_bytes,
                           int index_base, int64_t n_nodes, int64_t *offsets, void *s_out, void *t_out,
                           void *eid_out, int64_t capacity, int64_t *total, gnnmp_stream_t stream);

/* Edge coalescing (csrc/coalesce.hip) — the sort, mask and index map of remove_multi_edges(g; aggr), to_bidirected and to_unidirected
 * (GNNGraphs/src/transform.jl:157-185, 495-529), which the reference runs on the CPU.  Coalescing parallel edges is a bipartite plan
 * from the input edges to the output edges, and aggregating edge data over it is propagate(copy_xj, aggr): this call writes the output
 * edge list and that plan's CSC arrays, gnnmp_plan_from_csc(colptr, rowval, n_src = n_edges, n_dst = *total) makes the plan without
 * another sort, and gnnmp_propagate_f32(plan, GNNMP_COPY_XJ, aggr, edata) reduces [n_edges][D] edge data to [*total][D].
 *   mode  GNNMP_COALESCE_DIRECTED    key (s, t) over the n_edges input edges                                        E' = n_edges
 *         GNNMP_COALESCE_MIRRORED    the VIRTUAL list [s; t], [t; s] of to_bidirected (position p >= n_edges is edge p - n_edges
 *                                    reversed); the concatenation and the doubled edge data `[e e]` are never materialised   E' = 2 n_edges
 *         GNNMP_COALESCE_UNDIRECTED  key (min(s, t), max(s, t)), to_unidirected's encoding; the output edge is (lo, hi) itself.  The
 *                                    reference decodes its triangular index with a Float64 sqrt (utils.jl:244), which is exact only
 *                                    for small n; here nothing is encoded, so nothing is decoded.                     E' = n_edges
 * The virtual positions 0 .. E' - 1 are sorted STABLY by key (the reference's sortperm is stable); a key larger than its predecessor
 * starts an output edge.  The output is the distinct edges in ascending key order — lexicographic (s, t), the order of the reference's
 * (s - 1) n + t — and it is sorted whether or not any duplicate existed.  Written through the job (all device memory):
 *   s_out, t_out [0 .. *total)   the output edges, in the width and base of the inputs        (capacity E' each)
 *   colptr [0 .. *total]          the first sorted slot of every output edge, in index_base, ending at E' + index_base   (capacity E' + 1)
 *   rowval [0 .. E')              for every sorted slot, the row (in index_base) of the ORIGINAL edge data it came from: a virtual
 *                                 position p >= n_edges is folded to p - n_edges, so the mirrored copy reads the same row
 * and nothing else: no byte outside those ranges of any output.  *total is HOST memory.  Integer work only, no atomics on data:
 * bit-exact against the reference's algorithm.  Refused before any HIP call: GNNMP_EINVAL for a NULL job or total, idx_bytes not 4 | 8,
 * index_base not 0 | 1, an unknown mode, a negative size, a NULL pointer with n_edges > 0; GNNMP_EBOUNDS for n_nodes > 2^32 (indices
 * must fit 32 bits, as for gnnmp_sort_edge_index) or E' >= 2^32 (the pair sort's value width).  An index outside 0 .. n_nodes - 1 found
 * on the device is GNNMP_EBOUNDS too, with no output written.  n_edges = 0 returns GNNMP_OK with *total = 0 and touches nothing. */
typedef enum { GNNMP_COALESCE_DIRECTED = 0, GNNMP_COALESCE_MIRRORED = 1, GNNMP_COALESCE_UNDIRECTED = 2 } gnnmp_coalesce_mode;
typedef struct {
    const void *s;
    const void *t;
    int idx_bytes;
    int index_base;
    int64_t n_edges;
    int64_t n_nodes;
    int mode;
    void *s_out;
    void *t_out;
    void *colptr;
    void *rowval;
} gnnmp_coalesce_t;
/* Synchronises the stream (graph prep). */
int gnnmp_coalesce_edges(const gnnmp_coalesce_t *job, int64_t *total, gnnmp_stream_t stream);

/* Stable stream compaction of an edge list: the edges that satisfy the rule, in their original order.
 *   rule  GNNMP_COMPACT_SELF_LOOPS  keep s != t                          remove_self_loops(g)          transform.jl:49-64
 *         GNNMP_COMPACT_LIST        keep the positions that are NOT in `remove` (n_remove device entries in idx_bytes / index_base;
 *                                   a repeated position is harmless, one outside the edge list is GNNMP_EBOUNDS with no output
 *                                   written)                              remove_edges(g, idx)          transform.jl:121-139
 *         GNNMP_COMPACT_RANDOM      keep position e with probability 1 - p: kept when the 32 bits of gnnmp_dropout_keep_u8's hash of
 *                                   (seed, e, h = 0) are >= floor(p 2^32) (p = 1 keeps nothing) — a pure function of (seed, e), so
 *                                   the same seed gives the same graph whatever the launch shape; not Julia's RNG stream
 *                                                                         remove_edges(g, p)            transform.jl:142-146
 * Writes s_out, t_out, w_out (w and w_out both NULL, or both given: the kept weights) and eid_out — the kept positions, in index width
 * and base: edge features are then taken with gnnmp_gather_f32(edata, eid_out, ...) — entries [0 .. *total) of each, capacity n_edges;
 * nothing else is written.  *total is HOST memory.  Refused before any HIP call: GNNMP_EINVAL for a NULL job or total, bad idx_bytes /
 * index_base / rule, a negative size, p outside [0, 1], w without w_out or the reverse, a NULL pointer that would be dereferenced;
 * GNNMP_EBOUNDS for n_edges >= 2^32.  n_edges = 0 returns GNNMP_OK with *total = 0 and touches nothing. */
typedef enum { GNNMP_COMPACT_SELF_LOOPS = 0, GNNMP_COMPACT_LIST = 1, GNNMP_COMPACT_RANDOM = 2 } gnnmp_compact_rule;
typedef struct {
    const void *s;
    const void *t;
    const float *w;
    int idx_bytes;
    int index_base;
    int64_t n_edges;
    int rule;
    const void *remove;
    int64_t n_remove;
    float p;
    uint64_t seed;
    void *s_out;
    void *t_out;
    float *w_out;
    void *eid_out;
} gnnmp_compact_t;
/* Synchronises the stream (graph prep). */
int gnnmp_compact_edges(const gnnmp_compact_t *job, int64_t *total, gnnmp_stream_t stream);

/* has_multi_edges(g) — GNNGraphs/src/query.jl:575-579: fewer distinct (s, t) pairs than edges, i.e. two equal neighbours among the
 * sorted packed pairs; *result = 0 | 1 (host).  Indices must fit 32 bits (GNNMP_EBOUNDS otherwise).  Synchronises the stream. */
int gnnmp_has_multi_edges(const void *s, const void *t, int idx_bytes, int index_base, int64_t n_edges, int *result,
                          gnnmp_stream_t stream);
/* has_isolated_nodes(g; dir) — GNNGraphs/src/query.jl:420-422: any(iszero, degree(g; dir)), i.e. any empty row of the plan (dir = :in
 * the graph's plan, dir = :out the plan of the reversed edge index); *result = 0 | 1 (host).  The plan is only read.  Synchronises the
 * stream. */
int gnnmp_has_isolated_nodes(gnnmp_graph_t *plan, int *result, gnnmp_stream_t stream);

/* random_walk_pe(g, walk_length) — GNNGraphs/src/transform.jl:975-990: the random-walk positional encodings of every node,
 *   A = adjacency_matrix(g, Float32; dir = :out)   A[i, j] = the summed weights of the edges i -> j (1 per edge without weights)
 *   deg[i] = sum_j A[i, j], dinv = 1 ./ deg with Inf -> 0 (a node without out-edges), RW = A * Diagonal(dinv): RW[i, j] = A[i, j] dinv[j]
 *   pe[k, c] = (RW^k)[c, c],  k = 1 .. walk_length
 * The reference forms the N x N powers and keeps their diagonals.  Here column c of RW^k is k propagates of the unit vector e_c,
 *   v_k[i] = sum over the edges e: i -> j of (w_e * dinv[j]) * v_{k-1}[j]   (fp32, in original edge order, product then sum),
 * and a batched graph is block diagonal: a workgroup keeps the two [n_g][GNNMP_RWPE_TILE] panels of GNNMP_RWPE_TILE start nodes of one
 * member graph in LDS and writes only the encodings; a graph whose panels exceed the LDS budget (496 nodes by default) runs the same row
 * walk over panels in device scratch, with the same bits.  Deterministic, no atomics; bit-identical for a member graph alone and inside
 * any batch.
 *   plan_t      the TRANSPOSED plan of g (the plan of (t, s): a row holds the out-edges of a node) WITHOUT added self loops
 *   job         a host record of device pointers:
 *     w            [n_edges] edge weights in original edge order, or NULL
 *     graph_ptr    [n_graphs + 1] 0-based node offsets of the member graphs (idx_bytes 4 | 8; empty graphs allowed), or NULL: one graph
 *     out          [N][walk_length] — the memory of the reference's (walk_length, N) matrix — every element written, nothing else;
 *                  4-byte aligned
 * A set-up call like a plan build: it allocates scratch for the graphs of the scratch path and synchronises the stream.  With a graph_ptr
 * one check launch verifies that it ascends from 0 to N and that no edge leaves its graph's node range: GNNMP_EINVAL otherwise, with out
 * untouched.  Refused before any HIP call (GNNMP_EINVAL): a NULL plan_t, job or out, walk_length outside 1 .. GNNMP_RWPE_MAX_WALK,
 * idx_bytes not 4 | 8, n_graphs < 1 with a graph_ptr, a plan with added self loops or n_src != n_dst.  Float32 only; no adjoint (the
 * reference marks nothing differentiable here). */
#define GNNMP_RWPE_TILE 16
#define GNNMP_RWPE_MAX_WALK 1024
typedef struct {
    const float *w;
    const void *graph_ptr;
    int idx_bytes;
    int64_t n_graphs;
    int64_t walk_length;
    float *out;
} gnnmp_rwpe_t;
/* Synchronises the stream (graph prep). */
int gnnmp_random_walk_pe_f32(gnnmp_graph_t *plan_t, const gnnmp_rwpe_t *job, gnnmp_stream_t stream);

/* ppr_diffusion(g; alpha) — GNNGraphs/src/transform.jl:1026-1051: the personalised-PageRank re-weighting of the existing edges,
 *   A = sparse(t, s, w, N, N)          A[t, s] = the summed weights of the edges s -> t (1 per edge without weights), Float32
 *   M = I + (alpha32 - 1) * A          (the product is rounded, then added; alpha32 = alpha rounded to float32, used in both places)
 *   new_w[e] = alpha32 * inv(M)[t_e, s_e]        (every copy of a multi-edge receives the same value; no column is normalised)
 * The reference inverts the dense N x N matrix on the host.  A batched graph is block diagonal, so here every member graph of n nodes is
 * its own n x n block, inverted IN PLACE (n * n floats, no augmented [M | I]) by Gauss-Jordan elimination with partial pivoting:
 *   build    A[t][s] accumulates in slot order (the original edge order), then M[i][j] = delta_ij + (alpha32 - 1) * A[i][j]
 *   step k   f_i = a_ik for every row i.  The pivot row p is the row i >= k with the largest |f_i|, the LOWEST such i on a tie.  An
 *            exactly zero pivot marks the block singular and the step is skipped.  Otherwise rows p and k are exchanged, the pivot
 *            row becomes r_j = a_kj / piv with a_kk taken as 1 (so r_k = 1 / piv), and every other row i is updated as
 *              a_ij = fmaf(-f_i, r_j, a_ij)   for j != k,        a_ik = fmaf(-f_i, r_k, 0)
 *   finish   the row exchanges are undone on the columns, last first (an index map; no element moves or changes)
 *   write    out[eid] = alpha32 * Minv[t - base][s - base] for every slot of the member graph
 * Every element sees this one sequence of fp32 operations whichever path runs.  A member graph whose block, a column and the exchange
 * list ((n * n + 2 n) * 4 bytes) fit the LDS budget of a workgroup — 64 KB by default: n <= 127; at most 160 KB: n <= 201 — is
 * eliminated by one workgroup in LDS; a larger one in device scratch, one after another on the stream, every step a pivot launch
 * (search, exchange, scale) and a grid-wide update launch, the pivot index and the singular mark staying on the device.  The two paths,
 * a member graph alone and the same graph inside any batch give the same bits.  Deterministic.
 *   plan_t      the TRANSPOSED plan of g (the plan of (t, s): a row holds the out-edges of a node) WITHOUT added self loops
 *   job         a host record of device pointers:
 *     w                 [n_edges] edge weights in original edge order, or NULL (all ones)
 *     graph_ptr         [n_graphs + 1] 0-based node offsets of the member graphs (idx_bytes 4 | 8; empty graphs allowed), or NULL: one graph
 *     alpha             the damping factor
 *     lds_budget_bytes  0 = the default (64 KB); a smaller value sends more member graphs through the scratch path, values above
 *                       160 KB count as 160 KB
 *     out               [n_edges] the new weights in original edge order — every element written, nothing else; 4-byte aligned
 * A set-up call like a plan build: it allocates scratch (GNNMP_PPR_MAX_NODES^2 floats at most) and synchronises the stream.  With a
 * graph_ptr one check launch verifies that it ascends from 0 to N and that no edge leaves its graph's node range: GNNMP_EINVAL
 * otherwise, with out untouched.  Refused before any HIP call: (GNNMP_EINVAL) a NULL plan_t, job or out (with n_edges > 0), idx_bytes
 * not 4 | 8, n_graphs < 1 with a graph_ptr, a plan with added self loops or n_src != n_dst, a non-finite alpha, a negative
 * lds_budget_bytes.  A member graph of more than GNNMP_PPR_MAX_NODES nodes is GNNMP_EUNSUPPORTED (the dense n x n block: 64 MB of
 * scratch and 8192 launches at the limit), with out untouched.  A singular block — an exactly zero pivot after pivoting, the
 * reference's SingularException — is GNNMP_EINVAL after the final synchronisation; gnnmp_last_error names the first such member graph
 * and out is then UNSPECIFIED.  N == 0 or n_edges == 0: GNNMP_OK, nothing is launched.  Float32 only; no adjoint (the reference marks
 * nothing differentiable here). */
#define GNNMP_PPR_MAX_NODES 4096
typedef struct {
    const float *w;
    const void *graph_ptr;
    int idx_bytes;
    int64_t n_graphs;
    float alpha;
    int64_t lds_budget_bytes;
    float *out;
} gnnmp_ppr_t;
/* Synchronises the stream (graph prep). */
int gnnmp_ppr_diffusion_f32(gnnmp_graph_t *plan_t, const gnnmp_ppr_t *job, gnnmp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Leaf ops: _gather / _scatter (GNNGraphs/src/gatherscatter.jl:4,12-18)
 * ---------------------------------------------------------------------------------------------- */
/* out[k][:] = x[idx[k]][:]  for k in [0,K)  — NNlib.gather; pure copy, bit-exact. */
int gnnmp_gather_f32(const float *x, const void *idx, int idx_bytes, int index_base, int64_t K,
                     float *out, int64_t D, gnnmp_stream_t stream);
/* out[k][:] = xi[t_k][:] - xj[s_k][:]  (xj_minus_xi = 0: xi_sub_xj) or xj[s_k][:] - xi[t_k][:] (1: xj_sub_xi) for every
 * edge k — apply_edges with those message functions (GNNlib/src/msgpass.jl:177-185) without materialising the two
 * gathered (D, E) arrays.  (xi_dot_xj, :172, is gnnmp_edge_dot_f32 below.) */
int gnnmp_edge_sub_f32(const float *xi, const float *xj, const void *s, const void *t, int idx_bytes, int index_base,
                       int64_t K, int xj_minus_xi, float *out, int64_t D, gnnmp_stream_t stream);
/* out[i][:] = aggr_{k : t_k = i, in edge order} m[k][:]   — NNlib.scatter(aggr, m, t; dstsize=(D, n_dst))
 * with t = the plan's dst.  m is [E'][D] in ORIGINAL edge order (self-loop rows last). */
int gnnmp_scatter_f32(gnnmp_graph_t *plan, int aggr, const float *m, float *out, int64_t D,
                      gnnmp_stream_t stream);
/* What NNlib's KernelAbstractions scatter does on GPU arrays today: one atomic per element, fp32 '+'
 * order not defined.  Kept as the measured comparator and for callers that have no plan.
 * `out` must be pre-filled with the identity by the caller.  aggr in {SUM, MAX, MIN}. */
int gnnmp_scatter_atomic_f32(int aggr, const float *m, const void *idx, int idx_bytes,
                             int index_base, int64_t K, float *out, int64_t D,
                             gnnmp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Fused propagate  (GNNlib/src/msgpass.jl:71-79; fast-path specialisations :215-238)
 *
 *   out[i][:] = scale_dst[i] * aggr_{p in row i} ( w[eid_p] * ( scale_src[col_p] * xj[col_p][:] ) )
 *
 * msg = COPY_XJ ignores w.  w has n_edges entries in ORIGINAL edge order (self loops added by the plan
 * have weight 1, as GNNlib/src/layers/conv.jl:28-33 and transform.jl:22-24 pad).  scale_src / scale_dst
 * (nullable) are the GCN normalisation vectors `cout`, `cin` of GNNlib/src/layers/conv.jl:57-67; every
 * product is rounded separately (no FMA contraction) so the result equals the reference's materialised
 * `xj .* cout'` -> propagate -> `x .* cin'` sequence bit for bit on rows <= GNNMP_LONG_ROW.
 * ---------------------------------------------------------------------------------------------- */
int gnnmp_propagate_f32(gnnmp_graph_t *plan, int msg, int aggr, const float *xj, const float *w,
                        const float *scale_src, const float *scale_dst, float *out, int64_t D,
                        gnnmp_stream_t stream);

/* propagate(e_mul_xj, g, aggr; xj, e) with a MATRIX e of size (D, E) — GNNlib/src/msgpass.jl:187-191 (`e .* xj`): every
 * edge carries its own row of D factors, e[k][:] in original edge order.  out[i] = aggr_{k: t_k = i} e[k] .* xj[s_k];
 * edges the plan added as self loops weigh 1.  Two rows per edge are fetched (the factor row by edge id, the feature row
 * by source id); the (D, E') product is never written. */
int gnnmp_propagate_emul_f32(gnnmp_graph_t *plan, int aggr, const float *xj, const float *e, float *out, int64_t D,
                             gnnmp_stream_t stream);

/* The gated message of res_gated_graph_conv (GNNlib/src/layers/conv.jl:287-300):
 *   out[i] = aggr_{k: t_k = i} sigmoid.(gate_i[i] .+ Bx[s_k]) .* Vx[s_k]
 * gate_i = A*x [n_dst][D]; bv_j [n_src][2D] holds every source's Bx (first D) and Vx (last D) side by side — one dense
 * call with the stacked weight [B; V] produces it, and one contiguous 8D-byte gather per edge reads it.  sigmoid is
 * NNlib's formulation (exp(-|x|) based).  The (D, E) gate and message arrays are never written. */
int gnnmp_propagate_gated_f32(gnnmp_graph_t *plan, int aggr, const float *gate_i, const float *bv_j, float *out,
                              int64_t D, gnnmp_stream_t stream);

/* The same fused propagate with the per-edge factors already laid out in the plan's slot order:
 *   w_slot[p]   = w[eid_p]          (1 for plan-added self loops)      — gnnmp_plan_slot_gather_f32(plan, 1, w, ...)
 *   ss_slot[p]  = scale_src[col_p]                                    — gnnmp_plan_slot_gather_f32(plan, 0, scale_src, ...)
 * (either may be NULL).  The products and their order are identical to gnnmp_propagate_f32, hence so are the bits;
 * what changes is the traffic: a coalesced 4 B read per edge instead of a random 4 B gather (one 64 B sector) per
 * edge.  The factors depend only on the graph (GCN's 1/sqrt(deg), the graph's own weights), so a caller computes them
 * once per graph where the reference recomputes `xj .* cout'` on every call (GNNlib/src/layers/conv.jl:57-59). */
/* cg_conv's propagate (GNNlib/src/layers/conv.jl:304-333): out[i] = Σ_{j -> i} sigmoid(f_ij) .* act(s_ij) with
 *   z = vcat(x_i, x_j, e_ij),  f = l.dense_f's W z + b,  s = l.dense_s's W z + b  (act = dense_s's σ, any gnnmp_act)
 * split by the blocks of the two weight matrices: fs_i [n_dst][2D] = the x_i share of (f | s) with the biases folded in,
 * fs_j [n_src][2D] the x_j share, fs_e [n_edges][2D] the edge share in original edge order (NULL without edge features).
 * One pass over the edges; the (2D, E) pre-activations of the reference are never built. */
int gnnmp_propagate_cg_f32(gnnmp_graph_t *plan, const float *fs_i, const float *fs_j, const float *fs_e, int act,
                           float *out, int64_t D, gnnmp_stream_t stream);
/* nn_conv's propagate (GNNlib/src/layers/conv.jl:260-273): out[i] = aggr_{k: j -> i} W_k x_j with one (Dout, Din) matrix per
 * edge, W_k = reshape(l.nn(e)[:, k], Dout, Din) — `we` is nn(e) as the reference holds it, [n_edges][Dout * Din] in
 * original edge order, element (o, c) of edge k at we[k][o + Dout * c].  The (Dout, E) message array is never built. */
int gnnmp_propagate_nn_f32(gnnmp_graph_t *plan, int aggr, const float *xj, const float *we, float *out, int64_t Din,
                           int64_t Dout, gnnmp_stream_t stream);
int gnnmp_propagate_slots_f32(gnnmp_graph_t *plan, int aggr, const float *xj, const float *w_slot,
                              const float *ss_slot, const float *scale_dst, float *out, int64_t D,
                              gnnmp_stream_t stream);
/* the same with the layer epilogue of gcn_conv's W-first branch in the row kernel: out = act.(A .+ bias), A = what
 * gnnmp_propagate_slots_f32 returns — `x = l.weight * x` before the convolution when Dout < Din, then `σ.(x .+ l.bias)` after it
 * (GNNlib/src/layers/conv.jl:36-40,71).  bias: [D] or NULL; act: GNNMP_ACT_IDENTITY | GNNMP_ACT_RELU.  Bit-identical to
 * gnnmp_propagate_slots_f32 followed by gnnmp_bias_act_f32, one pass over (N, D) less. */
int gnnmp_propagate_slots_act_f32(gnnmp_graph_t *plan, int aggr, const float *xj, const float *w_slot, const float *ss_slot,
                                  const float *scale_dst, const float *bias, int act, float *out, int64_t D,
                                  gnnmp_stream_t stream);
/* out_slot[p] = v[col_p] (by = 0: v is a node vector of n_src entries) or v[eid_p] (by = 1: v is an edge vector of
 * n_edges entries in original order; plan-added self loops get 1.0).  out_slot has E' entries. */
int gnnmp_plan_slot_gather_f32(gnnmp_graph_t *plan, int by, const float *v, float *out_slot,
                               gnnmp_stream_t stream);

/* degree(g, Float32; dir = :in, edge_weight) — GNNGraphs/src/query.jl:314-331,355-369.
 * w == NULL: counts (exact integers).  w != NULL: n_edges weights in original order, summed in edge
 * order; plan-added self loops count 1. */
int gnnmp_degree_f32(gnnmp_graph_t *plan, const float *w, float *deg, gnnmp_stream_t stream);

/* out[i] = 1/sqrt(deg[i])  — the default norm_fn of GCNConv (GraphNeuralNetworks/src/layers/conv.jl:99);
 * evaluated as the correctly rounded sqrt then the correctly rounded division, like Julia's broadcast. */
int gnnmp_inv_sqrt_f32(const float *deg, float *out, int64_t n, gnnmp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * softmax_edge_neighbors(g, e) — GNNlib/src/utils.jl:84-97.  logits and alpha are [E'][H] in ORIGINAL
 * edge order.  Per destination and channel: max, exp(e - max), sum in edge order, true division.
 * ---------------------------------------------------------------------------------------------- */
int gnnmp_edge_softmax_f32(gnnmp_graph_t *plan, const float *logits, float *alpha, int64_t H,
                           gnnmp_stream_t stream);
/* softmax_nodes(g, x) / softmax_edges(g, e) — GNNlib/src/utils.jl:49-72: the same three steps over the segments of a
 * graph indicator.  plan = a plan whose destination index is the indicator (src = 1..K, dst = indicator, n_dst =
 * num_graphs); x, out [K][D] in original order.  den_add is added to the denominator when non-zero: softmax_edges
 * divides by `den .+ eps(T)` (utils.jl:71), softmax_nodes by `den` (utils.jl:57). */
int gnnmp_segment_softmax_f32(gnnmp_graph_t *plan, const float *x, float *out, int64_t D, float den_add,
                              gnnmp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * GATConv attention path — GNNlib/src/layers/conv.jl:112-167 from `apply_edges` to
 * `aggregate_neighbors`, fused.
 *   Wx       : [N][H][C]  (Julia reshape(dense_x(x), C, H, N))
 *   a        : [H][2C]    (Julia l.a of size (2C, H)); a[h][0:C] pairs with the TARGET Wx_i,
 *                          a[h][C:2C] with the SOURCE Wx_j (order of vcat(Wxi, Wxj), conv.jl:157)
 * gnnmp_gat_node_scores_f32: score_dst[n][h] = sum_c a[h][c]*Wx[n][h][c],
 *                            score_src[n][h] = sum_c a[h][C+c]*Wx[n][h][c]   (either out may be NULL)
 * gnnmp_gat_aggregate_f32  : logit_p[h] = leakyrelu(score_dst[i][h] + score_src[col_p][h], slope)
 *                            alpha = softmax over row i (as gnnmp_edge_softmax_f32)
 *                            out[i][h][:] = sum_p alpha_p[h] * Wx_src[col_p][h][:]   (edge order)
 *   alpha_out (nullable): [E'][H] attention coefficients in original edge order.
 *   bias (nullable, [H*C]) and act: the layer's `σ.(x .+ bias)` (conv.jl:147) fused into the store for the
 *   concat = true case.
 * ---------------------------------------------------------------------------------------------- */
int gnnmp_gat_node_scores_f32(const float *Wx, const float *a, float *score_dst, float *score_src,
                              int64_t N, int64_t H, int64_t C, gnnmp_stream_t stream);
int gnnmp_gat_aggregate_f32(gnnmp_graph_t *plan, const float *Wx_src, const float *score_dst,
                            const float *score_src, float negative_slope, const float *bias, int act,
                            float *out, float *alpha_out, int64_t H, int64_t C,
                            gnnmp_stream_t stream);

/* The production entry point for the same GATConv path: ONE pass over the edges, no node pre-pass, no score arrays.
 * The source half of the logit is formed in registers from the source row that the weighted sum fetches anyway, the
 * target half from row i of Wx_dst (NULL = Wx_src), and the neighbourhood softmax is computed online (running max and
 * denominator).  Same mathematical function as gnnmp_gat_node_scores_f32 + gnnmp_gat_aggregate_f32; rounding differs
 * at the 1e-6 level (north_star's bar for fp32 aggregation is 1e-5).  Head widths whose lane count is not a power of
 * two fall back to those two kernels internally (scores in the plan's workspace). */
int gnnmp_gat_conv_f32(gnnmp_graph_t *plan, const float *Wx_src, const float *Wx_dst, const float *a,
                       float negative_slope, const float *bias, int act, float *out, int64_t H,
                       int64_t C, gnnmp_stream_t stream);

/* gat_conv with edge features (l.dense_e, conv.jl:152-167: `Wxx = vcat(Wxi, Wxj, We)`): the edge's share of the logit,
 * edge_score[k][h] = a[2C:3C, h] . We_k[:, h] with We = dense_e(e), is a per-edge scalar per head — compute it with
 * gnnmp_gat_node_scores_f32 on the (E, H*C) matrix We — and is added inside the one-pass kernel, fetched by original edge
 * position.  `a` is the node part [H][2C].  The plan must not add self loops (conv.jl:119-121 forbids the combination). */
int gnnmp_gat_conv_edge_f32(gnnmp_graph_t *plan, const float *Wx_src, const float *Wx_dst, const float *a,
                            const float *edge_score, float negative_slope, const float *bias, int act, float *out,
                            int64_t H, int64_t C, gnnmp_stream_t stream);

/* Training forward of the same path: as gnnmp_gat_conv_f32, and additionally saves the neighbourhood-softmax statistics
 * stats[i][h] = (m_i, den_i) — the running maximum of the logits and Σ_j exp(l_ij - m_i) — 8 bytes per destination and
 * head instead of the reference's (H, E') α array that Zygote keeps alive for the pullback.  The feature row must fit one
 * wave (H*C / v lanes <= 64 with v = 4, 2 or 1 floats per lane as C's divisibility AND the alignment of the [.][H*C] arrays allow:
 * v = 4 needs C % 4 == 0 and every such array of the call 16-byte aligned, v = 2 needs C % 2 == 0 and 8-byte alignment, any float-aligned
 * pointer runs with v = 1; GNNMP_EUNSUPPORTED otherwise — so a row of more than 64 floats is refused when a pointer is under-aligned
 * for the v it needs).  The same rule holds for every one-pass attention entry point and pullback below (gnnmp_gat_conv_edge_f32 /
 * _train_f32 / _drop_f32, gnnmp_attn_conv_f32 / _drop_f32, gnnmp_gat_conv_grad_f32 / _grad2_f32 / _grad_drop_f32, gnnmp_attn_conv_grad_f32 /
 * _grad_drop_f32, gnnmp_attn_conv_edge_f32 / _edge_grad_f32: out, oplus, dout, F, dF and the [.][H*C] gradient arrays count); gnnmp_gat_conv_f32 falls back to the three-pass kernels instead.
 * Head widths whose lane count is a power of two reduce with DPP butterflies; any other width (C = 7 classes, ...) is
 * supported too, summing the head's lanes one by one. */
int gnnmp_gat_conv_stats_f32(gnnmp_graph_t *plan, const float *Wx_src, const float *Wx_dst, const float *a,
                             float negative_slope, const float *bias, int act, float *out, float *stats,
                             int64_t H, int64_t C, gnnmp_stream_t stream);

/* Dropout on the attention coefficients — GNNlib/src/layers/conv.jl:139 `α = dropout(α, l.dropout)` (NNlib.dropout: every
 * coefficient kept with probability 1 - p and scaled by 1 / (1 - p); the reference applies it whenever l.dropout > 0).  Inside the
 * one-pass kernel: out_i = Σ_j keep_ij / (1 - p) α_ij Wx_j with α the UNdropped softmax, so the saved statistics (stats, nullable) are
 * those of gnnmp_gat_conv_stats_f32.  No mask is stored: keep_ij[h] is a pure function of (seed, e, h) that the forward, both
 * backward passes and a host restatement share —
 *     mix(x):  x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16     (32-bit, wrapping)
 *     keep  =  mix( mix(e ^ lo32(seed)) ^ (h * 0x9e3779b9 + hi32(seed)) )  >=  floor(p * 2^32)
 * with e = the edge's 0-based position in the caller's edge list (plan-added self loops: E + node, the order add_self_loops appends
 * them in) and h the 0-based head.  0 <= p < 1; p = 0 is gnnmp_gat_conv_stats_f32 / gnnmp_gat_conv_f32 exactly.  The feature row must
 * fit one wave and there are no edge features (GNNMP_EUNSUPPORTED otherwise).  A fresh seed per call gives the reference's behaviour;
 * the same seed must be handed to gnnmp_gat_conv_grad_drop_f32.
 * gnnmp_dropout_keep_u8 writes that mask, keep[e][h] in {0, 1}, for n_edges edge positions (tests, or a caller that wants α .* mask). */
/* The TRAINING forward of GATConv and its pullback with ONE edge pass (round 4).  With o_i = Σ_j α_ij Wx_j the softmax rrule's
 * D_i = Σ_j α_ij (Δ_i . Wx_j) is Δ_i . o_i, and dsd_i = Σ_j α_ij (g_ij - D_i) lrelu'(z_ij) = (1 - slope) (Δ_i . o+_i - D_i P_i) with
 * o+_i / P_i the same sums restricted to the edges whose logit z_ij is positive — so the forward also writes oplus [n_dst][H*C] and pplus
 * [n_dst][H] (4 bytes per feature and node more), and the destination side of the pullback becomes a node kernel on (dout, out, oplus,
 * pplus): the gather of every Wx_j by destination (5.7 ms on the products shape) is gone; the source-side pass, dWx, dss, da are those of
 * gnnmp_gat_conv_grad_f32.  `out` / `bias` of grad2 are the forward's output act(o + bias) and its bias (act = identity | relu): o is read
 * back as out - bias, which is exact wherever dout is not zero when dout = dL/d(o + bias) (relu's switched-off entries carry dout = 0).
 * No dropout, no edge features (those keep gnnmp_gat_conv_stats_f32 / gnnmp_gat_conv_grad_f32). */
int gnnmp_gat_conv_train_f32(gnnmp_graph_t *plan, const float *Wx_src, const float *Wx_dst, const float *a, float negative_slope,
                             const float *bias, int act, float *out, float *stats, float *oplus, float *pplus, int64_t H, int64_t C,
                             gnnmp_stream_t stream);
int gnnmp_gat_conv_grad2_f32(gnnmp_graph_t *plan, gnnmp_graph_t *plan_t, const float *Wx_src, const float *Wx_dst, const float *a,
                             float negative_slope, const float *stats, const float *out, const float *bias, const float *oplus,
                             const float *pplus, const float *dout, float *line, float *dsd, float *dss, float *dWx_src, float *dWx_dst,
                             float *da, int64_t H, int64_t C, gnnmp_stream_t stream);
int gnnmp_gat_conv_drop_f32(gnnmp_graph_t *plan, const float *Wx_src, const float *Wx_dst, const float *a,
                            float negative_slope, float p, uint64_t seed, const float *bias, int act, float *out,
                            float *stats, int64_t H, int64_t C, gnnmp_stream_t stream);
int gnnmp_dropout_keep_u8(uint64_t seed, float p, int64_t n_edges, int64_t H, uint8_t *keep, gnnmp_stream_t stream);

/* The same one-pass kernel for the other attention layers that share the path: GATv2Conv
 * (gatv2_conv, conv.jl:171-214), TransformerConv's attention core (transformer_conv, conv.jl:553-616) and AGNNConv
 * (agnn_conv, conv.jl:337-352).  out[i][h][:] = Σ_j softmax_{j in N(i)}(l_ij) V_j[h][:], then + bias and act.
 *   Q [n_dst][H*C] (NULL = K), K [n_src][H*C], V [n_src][H*C] (NULL = K; a separate V only with GNNMP_ATTN_DOT)
 *   a: GAT [H][2C], GATV2 [H][C] (Julia (C, H) as stored), otherwise ignored
 *   scale: DOT divides the dot product by it (l.sqrt_out); COS multiplies the cosine by it (l.β); else ignored
 *   stats: optional [n_dst][H][2] softmax statistics as in gnnmp_gat_conv_stats_f32
 * The feature row must fit one wave (see gnnmp_gat_conv_stats_f32); GNNMP_EUNSUPPORTED otherwise (mode GAT without stats
 * falls back to the three-pass kernels instead). */
int gnnmp_attn_conv_f32(gnnmp_graph_t *plan, int mode, const float *Q, const float *K, const float *V,
                        const float *a, float negative_slope, float scale, const float *bias, int act,
                        float *out, float *stats, int64_t H, int64_t C, gnnmp_stream_t stream);

/* Pullback of the attention path (what Zygote composes from the rrules of gather / leakyrelu / softmax_edge_neighbors /
 * scatter(+) for conv.jl:136-141,152-167).  dout = Δ w.r.t. the aggregated (pre-bias, pre-σ) output [n_dst][H*C];
 * plan_t = plan of the reversed edge index (same self-loop flag); stats from gnnmp_gat_conv_stats_f32.
 * Scratch/outputs supplied by the caller: line [n_dst][H][4] (16-byte aligned), dsd [n_dst][H] (Δ of the target logit
 * half), dss [n_src][H] (Δ of the source half).  Results: dWx_src [n_src][H*C]; dWx_dst [n_dst][H*C] for a bipartite
 * layer (Wx_dst != Wx_src) — with Wx_dst NULL / == Wx_src pass dWx_dst = NULL and dWx_src holds the whole ΔWx;
 * da [H][2C] (may be NULL).  Two passes over the edges, no atomics, run-to-run identical. */
int gnnmp_gat_conv_grad_f32(gnnmp_graph_t *plan, gnnmp_graph_t *plan_t, const float *Wx_src, const float *Wx_dst,
                            const float *a, float negative_slope, const float *stats, const float *dout,
                            float *line, float *dsd, float *dss, float *dWx_src, float *dWx_dst, float *da,
                            int64_t H, int64_t C, gnnmp_stream_t stream);

/* The same pullback through the dropped coefficients of gnnmp_gat_conv_drop_f32 (same p and seed as the forward): with
 * k_ij = keep_ij / (1 - p), g_ij = k_ij (Δ_i . Wx_j) replaces Δ_i . Wx_j and Σ_i k_ij α_ij Δ_i replaces Σ_i α_ij Δ_i; everything else,
 * including the caller-supplied buffers, is as in gnnmp_gat_conv_grad_f32. */
int gnnmp_gat_conv_grad_drop_f32(gnnmp_graph_t *plan, gnnmp_graph_t *plan_t, const float *Wx_src, const float *Wx_dst,
                                 const float *a, float negative_slope, float p, uint64_t seed, const float *stats,
                                 const float *dout, float *line, float *dsd, float *dss, float *dWx_src, float *dWx_dst,
                                 float *da, int64_t H, int64_t C, gnnmp_stream_t stream);

/* gnnmp_attn_conv_f32 with dropout on the attention coefficients — gatv2_conv's `α = dropout(α, l.dropout)` (conv.jl:191); same mask
 * function, same rules as gnnmp_gat_conv_drop_f32 (mode GNNMP_ATTN_GAT or GNNMP_ATTN_GATV2; GNNMP_EUNSUPPORTED for the others, which
 * have no dropout in the reference), and its pullback for the GATV2 logit (same p and seed; arguments as gnnmp_attn_conv_grad_f32). */
int gnnmp_attn_conv_drop_f32(gnnmp_graph_t *plan, int mode, const float *Q, const float *K, const float *V, const float *a,
                             float negative_slope, float scale, float p, uint64_t seed, const float *bias, int act, float *out,
                             float *stats, int64_t H, int64_t C, gnnmp_stream_t stream);
int gnnmp_attn_conv_grad_drop_f32(gnnmp_graph_t *plan, gnnmp_graph_t *plan_t, int mode, const float *Q, const float *K,
                                  const float *V, const float *a, float negative_slope, float scale, float p, uint64_t seed,
                                  const float *stats, const float *dout, float *line, float *dQ, float *dK, float *dV, float *dA,
                                  float *da, int64_t H, int64_t C, gnnmp_stream_t stream);

/* Pullback of gnnmp_attn_conv_f32 for the GATV2 and DOT logits (the GAT logit has the cheaper dedicated entry above; the
 * cosine logit has none yet: GNNMP_EUNSUPPORTED).  dout = Δ w.r.t. the aggregated (pre-bias, pre-σ) output; stats from the
 * forward; plan_t = plan of the reversed edge index.  Caller-supplied: line [n_dst][H][4] (16-byte aligned scratch),
 * dQ [n_dst][H*C], dK [n_src][H*C]; DOT also dV [n_src][H*C]; GATV2 also dA [n_dst][H*C] (scratch: per-destination terms
 * of Δa) and da [H][C] (may be NULL).  With GATV2, V is K and dK holds the whole gradient of K.  Two edge passes, no
 * atomics, run-to-run identical. */
int gnnmp_attn_conv_grad_f32(gnnmp_graph_t *plan, gnnmp_graph_t *plan_t, int mode, const float *Q, const float *K,
                             const float *V, const float *a, float negative_slope, float scale, const float *stats,
                             const float *dout, float *line, float *dQ, float *dK, float *dV, float *dA, float *da,
                             int64_t H, int64_t C, gnnmp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Attention with a per-edge feature ROW, forward and pullback — gatv2_conv and transformer_conv with `e`, GNNlib/src/layers/conv.jl:171-214
 * and :553-629 (csrc/attn_edge.hip).  F = dense_e(e) | W6(e), [n_edges][H*C] in ORIGINAL edge order (gnnmp_dense_f32 on the E rows of e);
 * k = the original position of edge j -> i.  Per head, α_ij = softmax_{j in N(i)} l_ij:
 *   GNNMP_ATTN_GATV2   z_c = (Q_ic + K_jc) + F_kc,  l_ij = Σ_c a_c leakyrelu(z_c),   o_i = Σ_j α_ij K_j       (the value carries no F: gatv2_message)
 *   GNNMP_ATTN_DOT     l_ij = Q_i . (K_j + F_k) / scale,                              o_i = Σ_j α_ij (V_j + F_k) (transformer_message_uij / _main)
 *   gnnmp_attn_conv_edge_f32        out = act(o + bias) (act = identity | relu, bias nullable), stats[i][h] = (m_i, den_i) as in
 *                                   gnnmp_gat_conv_stats_f32 when the pointer is non-NULL.  One pass over the plan, online softmax; a row
 *                                   without in-edges gets o_i = 0 and stats (-Inf, 0).
 *   gnnmp_attn_conv_edge_grad_f32   dout = Δ w.r.t. o.  With g_ij = Δ_i . val_ij (val = K_j | V_j + F_k), D_i = Σ_j α_ij g_ij,
 *                                   dl_ij = α_ij (g_ij - D_i), s_c = leakyrelu'(z_c), α rebuilt from stats:
 *                                     GATV2  dQ_ic = a_c Σ_j dl_ij s_c,  dK_jc = Σ_i (a_c dl_ij s_c + α_ij Δ_ic)  (V is K: the whole gradient),
 *                                            dF_kc = a_c dl_ij s_c,  dA_ic = Σ_j dl_ij leakyrelu(z_c),  da_c = Σ_i dA_ic (rows in order, then a tree)
 *                                     DOT    dQ_i = Σ_j dl_ij (K_j + F_k) / scale,  dK_j = Σ_i dl_ij Q_i / scale,  dV_j = Σ_i α_ij Δ_i,
 *                                            dF_k = dl_ij Q_i / scale + α_ij Δ_i
 *                                   Pass 1 over plan: D_i, dQ_i, dA_i and the line (m, 1/den, D, 0) per (i, h); pass 2 over plan_t: dK_j, dV_j
 *                                   and dF_k, ONE plain store at the slot's original edge position — an edge is exactly one slot there.
 *   plan, plan_t   the graph's plan and the plan of the reversed edge index, both built WITHOUT plan-added self loops (conv.jl:178-181
 *                  forbids edge features with add_self_loops; F has no row for them).  They are only READ and their chunks are ignored:
 *                  every row is walked whole by one lane group, in slot order — no plan scratch, no atomics, every output element written
 *                  exactly once, two calls give equal bits, and a capture needs no eager call first.  A hub row is therefore slow.
 *   job            a const HOST record of device pointers.  Q NULL = K; V NULL = K (a separate V only with DOT).  The gradient record
 *                  carries the forward's inputs, its stats, dout, the caller's scratch line [n_dst][H][4] (16-byte aligned) and the
 *                  outputs dQ [n_dst][H*C], dK [n_src][H*C], dF [n_edges][H*C]; DOT: dV [n_src][H*C]; GATV2: dA [n_dst][H*C] and da [H][C]
 *                  (da nullable).  Every element of every output is written.
 * The feature row must fit one wave under the rule of gnnmp_gat_conv_stats_f32; F and dF count among the [.][H*C] arrays whose alignment
 * selects v (GNNMP_EUNSUPPORTED otherwise).  n_edges = 0: the forward writes act(bias) and the empty statistics, the pullback zero dQ, dK,
 * dV (dA, da) and the line; F and dF may be NULL.  Refused with GNNMP_EINVAL before any HIP call: a NULL plan, job or required pointer; a
 * NULL F (dF) with n_edges > 0; a mode other than GATV2 / DOT; H or C < 1 or H*C > 2^20; an act other than identity / relu; a plan built
 * with self loops; a plan_t that is not the plan's transpose; a separate V with GATV2; a line that is not 16-byte aligned.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
    const float *Q;    /* [n_dst][H*C] or NULL (= K) */
    const float *K;    /* [n_src][H*C] */
    const float *V;    /* [n_src][H*C] or NULL (= K); separate only with DOT */
    const float *F;    /* [n_edges][H*C], original edge order */
    const float *a;    /* GATV2: [H][C] */
    const float *bias; /* [H*C] or NULL */
    float *out;        /* [n_dst][H*C] */
    float *stats;      /* [n_dst][H][2] or NULL */
    float negative_slope;
    float scale;
    int act;
} gnnmp_attn_edge_t;
int gnnmp_attn_conv_edge_f32(const gnnmp_graph_t *plan, int mode, const gnnmp_attn_edge_t *job, int64_t H, int64_t C,
                             gnnmp_stream_t stream);

typedef struct {
    const float *Q;     /* as in the forward */
    const float *K;
    const float *V;
    const float *F;
    const float *a;
    const float *stats; /* [n_dst][H][2], from the forward */
    const float *dout;  /* [n_dst][H*C] */
    float *line;        /* [n_dst][H][4], 16-byte aligned scratch */
    float *dQ;          /* [n_dst][H*C] */
    float *dK;          /* [n_src][H*C] */
    float *dV;          /* DOT: [n_src][H*C] */
    float *dF;          /* [n_edges][H*C] */
    float *dA;          /* GATV2: [n_dst][H*C] */
    float *da;          /* GATV2: [H][C] or NULL */
    float negative_slope;
    float scale;
} gnnmp_attn_edge_grad_t;
int gnnmp_attn_conv_edge_grad_f32(const gnnmp_graph_t *plan, const gnnmp_graph_t *plan_t, int mode, const gnnmp_attn_edge_grad_t *job,
                                  int64_t H, int64_t C, gnnmp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Training GATConv with edge features — gat_conv with `e`, GNNlib/src/layers/conv.jl:112-167 (csrc/gat_backward.hip; the forward is
 * csrc/gat_fused.hip).  Per head h, for edge k = (j -> i) at its ORIGINAL position k, with a_d = a[h][0:C], a_s = a[h][C:2C] and
 * es_k[h] = a_e[h] . We_k[h] the edge's share of the logit (We = dense_e(e), a_e the edge third of the layer's `a`):
 *     z_ij = (a_d . Wx_dst_i + a_s . Wx_src_j) + es_k,  l_ij = leakyrelu(z_ij),  α_ij = softmax_{j in N(i)} l_ij,  o_i = Σ_j α_ij Wx_src_j
 *   gnnmp_gat_conv_edge_stats_f32   gnnmp_gat_conv_edge_f32 that also writes stats[i][h] = (m_i, den_i) as gnnmp_gat_conv_stats_f32 does when
 *                                   the pointer is non-NULL: the training forward.  The same kernels, the same bits in `out`.  The feature
 *                                   row must fit one wave (GNNMP_EUNSUPPORTED otherwise) and the plan must not add self loops (GNNMP_EINVAL).
 *   gnnmp_gat_conv_edge_grad_f32    dout = Δ w.r.t. o.  With g_ij = Δ_i . Wx_src_j, D_i = Σ_j α_ij g_ij and α rebuilt from stats:
 *                                     dz_ij = α_ij (g_ij - D_i) leakyrelu'(z_ij),  dsd_i = Σ_j dz_ij,  dss_j = Σ_i dz_ij,  dscore[k][h] = dz_ij,
 *                                     dWx_src_j = Σ_i α_ij Δ_i + a_s dss_j (+ a_d dsd_j when Wx_dst is Wx_src),  dWx_dst_i = a_d dsd_i,
 *                                     da[h] = (Σ_i dsd_i Wx_dst_i, Σ_j dss_j Wx_src_j)
 *                                   — gnnmp_gat_conv_grad_f32's two passes with es_k inside z: pass 1 over plan (D_i, dsd_i, the line), pass 2
 *                                   over plan_t (dWx_src, dss, and dscore: ONE plain store at the slot's original edge position — an edge is
 *                                   exactly one slot there, so every element of dscore is written exactly once).  Rows longer than the plans'
 *                                   threshold are chunked and folded in chunk order as in gnnmp_gat_conv_grad_f32; no atomics, two calls
 *                                   give equal bits.
 *                                   job: a const HOST record of device pointers.  Wx_dst NULL = Wx_src, and dWx_dst is NULL exactly then;
 *                                   edge_score [n_edges][H] in original edge order; stats from the forward; line [n_dst][H][4] 16-byte
 *                                   aligned scratch; dsd [n_dst][H], dss [n_src][H], dWx_src [n_src][H*C], dWx_dst [n_dst][H*C],
 *                                   dscore [n_edges][H] written in full; da [H][2C] nullable.  plan_t = the plan of the reversed edge index.
 *                                   n_edges = 0: zero dWx, dsd, dss and da and the line are written; edge_score and dscore may be NULL.
 *                                   Refused with GNNMP_EINVAL before any HIP call: a NULL plan, plan_t, job or required pointer; a NULL
 *                                   edge_score or dscore with n_edges > 0; H or C < 1 or H*C > 2^20; a plan built with self loops
 *                                   (conv.jl:119-121 forbids them with edge features; edge_score has no row for them); a plan_t that is not the
 *                                   plan's transpose; a bipartite plan without Wx_dst; a line that is not 16-byte aligned.  GNNMP_EUNSUPPORTED:
 *                                   a feature row that does not fit one wave under the rule of gnnmp_gat_conv_stats_f32.
 *   gnnmp_gat_edge_fold_f32         M[h][:] = Σ_c a_e[h][c] W_e[hC + c][:], [H][ein] from a_e [H][C] and dense_e's weight W_e [H*C][ein], c in
 *                                   order.  Then es = e M' (gnnmp_dense_f32 on the E rows of e, weight M), de = dscore M and dM = dscore' e
 *                                   (the dense adjoints): training never forms the [n_edges][H*C] array We.
 *   gnnmp_gat_edge_fold_grad_f32    dW_e[hC + c][:] = a_e[h][c] dM[h][:] and da_e[h][c] = dM[h] . W_e[hC + c] (k in order); dW_e or da_e may be
 *                                   NULL, and with both NULL nothing is launched.
 * Both fold calls only launch; GNNMP_EINVAL for H, C or ein < 1 (or above 2^20) and for a NULL required pointer.  Not here: attention
 * dropout together with edge features, Float64, the o+ / P shortcut of gnnmp_gat_conv_grad2_f32.
 * ---------------------------------------------------------------------------------------------- */
int gnnmp_gat_conv_edge_stats_f32(gnnmp_graph_t *plan, const float *Wx_src, const float *Wx_dst, const float *a,
                                  const float *edge_score, float negative_slope, const float *bias, int act, float *out,
                                  float *stats, int64_t H, int64_t C, gnnmp_stream_t stream);
typedef struct {
    const float *Wx_src;     /* [n_src][H*C] */
    const float *Wx_dst;     /* [n_dst][H*C] or NULL (= Wx_src) */
    const float *a;          /* [H][2C] */
    const float *edge_score; /* [n_edges][H], original edge order */
    const float *stats;      /* [n_dst][H][2], from the forward */
    const float *dout;       /* [n_dst][H*C] */
    float *line;             /* [n_dst][H][4], 16-byte aligned scratch */
    float *dsd;              /* [n_dst][H] */
    float *dss;              /* [n_src][H] */
    float *dWx_src;          /* [n_src][H*C] */
    float *dWx_dst;          /* [n_dst][H*C]; NULL exactly when Wx_dst is NULL or Wx_src */
    float *da;               /* [H][2C] or NULL */
    float *dscore;           /* [n_edges][H], original edge order */
    float negative_slope;
} gnnmp_gat_edge_grad_t;
int gnnmp_gat_conv_edge_grad_f32(gnnmp_graph_t *plan, gnnmp_graph_t *plan_t, const gnnmp_gat_edge_grad_t *job, int64_t H, int64_t C,
                                 gnnmp_stream_t stream);
int gnnmp_gat_edge_fold_f32(const float *a_e, const float *W_e, float *M, int64_t H, int64_t C, int64_t ein, gnnmp_stream_t stream);
int gnnmp_gat_edge_fold_grad_f32(const float *a_e, const float *W_e, const float *dM, float *dW_e, float *da_e, int64_t H, int64_t C,
                                 int64_t ein, gnnmp_stream_t stream);

/* out[n][c] = act( mean_h y[n][h][c] + bias[c] ) — the concat = false tail of gat_conv (`mean(x, dims = 2)`,
 * GNNlib/src/layers/conv.jl:143-147): heads added in order, one division by H, then σ.(x .+ bias). */
int gnnmp_head_mean_f32(const float *y, const float *bias, int act, float *out, int64_t N, int64_t H,
                        int64_t C, gnnmp_stream_t stream);
/* its pullback: dy[n][h][c] = dz[n][c] / H (the heads' gradient of `mean(x, dims = 2)`) */
int gnnmp_head_mean_grad_f32(const float *dz, float *dy, int64_t N, int64_t H, int64_t C, gnnmp_stream_t stream);
/* gmm_conv's mixture weights (GNNlib/src/layers/conv.jl:379-385): out[e][k * C + c] = exp(Σ_d ((e[e][d] - mu[k][d])^2 / 2) *
 * sigma_inv[k][d]^2) for every edge, kernel k and (repeated) output channel c — the factor array of the layer's
 * `propagate(e_mul_xj, g, mean; xj = reshape(dense_x(x), out, K, :), e = w)`, ready for gnnmp_propagate_emul_f32.
 * mu, sigma_inv: Julia (ein, K) column-major = [K][ein]. */
int gnnmp_gmm_weights_f32(const float *e, const float *mu, const float *sigma_inv, float *out, int64_t E, int64_t ein,
                          int64_t K, int64_t C, gnnmp_stream_t stream);
/* egnn_conv's radial features (GNNlib/src/layers/conv.jl:465-467): sq[k] = sum(x_diff[k][:] .^ 2) and
 * xn[k][:] = x_diff[k][:] / (sqrt(sq[k]) + eps) for every row k (eps = 1f-6 in the reference). */
int gnnmp_row_sqnorm_normalize_f32(const float *x, float *sq, float *xn, float eps, int64_t N, int64_t D,
                                   gnnmp_stream_t stream);
/* Flux.LSTMCell's pointwise part — the cell of set2set_pool (GNNlib/src/layers/pool.jl:31-44): gx = Wi x and gh = Wh h are
 * [N][4D] (gates input, forget, cell, output), b [4D] or NULL:
 *   c_out = σ(forget) .* c + σ(input) .* tanh(cell),  h_out = σ(output) .* tanh(c_out) */
int gnnmp_lstm_pointwise_f32(const float *gx, const float *gh, const float *b, const float *c, float *h_out, float *c_out,
                             int64_t N, int64_t D, gnnmp_stream_t stream);
/* out[n] = sum(a[n][:] .* b[n][:]) — `sum(qn .* x, dims = 1)` of set2set_pool (pool.jl:39) */
int gnnmp_rowdot_f32(const float *a, const float *b, float *out, int64_t N, int64_t D, gnnmp_stream_t stream);
/* Flux.GRUCell's pointwise part — the cell of gated_graph_conv (GNNlib/src/layers/conv.jl:228-232): gx = Wi m and
 * gh = Wh h are [N][3D] (gates r, z, candidate), b [3D] or NULL:
 *   r = σ(gx_r + gh_r + b_r), z = σ(gx_z + gh_z + b_z), h~ = tanh(gx_n + r .* gh_n + b_n), out = (1 - z) .* h~ + z .* h */
int gnnmp_gru_pointwise_f32(const float *gx, const float *gh, const float *b, const float *h, float *out, int64_t N,
                            int64_t D, gnnmp_stream_t stream);
/* xn[n][:] = x[n][:] / sqrt(sum(x[n][:]^2)) — `xn = x ./ sqrt.(sum(x .^ 2, dims = 1))` of agnn_conv
 * (GNNlib/src/layers/conv.jl:341-342); rnorm (optional) keeps the norms for the pullback.  A zero row gives NaN like the
 * reference's 0 / 0. */
int gnnmp_row_normalize_f32(const float *x, float *xn, float *rnorm, int64_t N, int64_t D, gnnmp_stream_t stream);
/* its pullback for the two uses of xn in the attention (query and key cotangents dq, dk; either may be NULL):
 *   dn = dq + dk;  dx = base + (dn - xn (xn . dn)) / rnorm   (base optional: another cotangent of x, e.g. the value's);
 *   qdot[n] = qscale (xn[n] . dq[n]) (optional): with logit = β (xn_i . xn_j) and qscale = 1 / β, Σ_n qdot[n] = dL/dβ. */
int gnnmp_row_normalize_grad_f32(const float *dq, const float *dk, const float *xn, const float *rnorm,
                                 const float *base, float *dx, float *qdot, float qscale, int64_t N, int64_t D,
                                 gnnmp_stream_t stream);
/* out = a + b (n floats) — degree(g; dir = :both) = out-degree + in-degree (GNNGraphs/src/query.jl:362-367). */
int gnnmp_add_f32(const float *a, const float *b, float *out, int64_t n, gnnmp_stream_t stream);
/* out[n][:] = a[n][:] .* b[n][:] with a of 1 channel (broadcast) or D channels — `α .* l.ffeat(x)` of
 * global_attention_pool, GNNlib/src/layers/pool.jl:6-10 (out may alias b) */
int gnnmp_mul_rows_f32(const float *a, int64_t Da, const float *b, float *out, int64_t N, int64_t D,
                       gnnmp_stream_t stream);
/* out = alpha .* x .+ y (out may alias x or y) — `(1 .+ ϵ) .* xi .+ m` of gin_conv, GNNlib/src/layers/conv.jl:250-256 */
int gnnmp_axpy_f32(float alpha, const float *x, const float *y, float *out, int64_t n, gnnmp_stream_t stream);
/* *result_host = 1 iff idx[0..n) is non-decreasing (is a graph_indicator one that `batch` could have built?).
 * Synchronises the stream (graph prep). */
int gnnmp_is_sorted(const void *idx, int idx_bytes, int64_t n, int *result_host, gnnmp_stream_t stream);

/* out[n][:] = act(x[n][:] + bias[:])  — the `σ.(x .+ bias)` tail of a layer body when it is not fused into
 * the producing kernel (GNNlib/src/layers/conv.jl:71,147).  bias nullable; out may alias x. */
int gnnmp_bias_act_f32(const float *x, const float *bias, int act, float *out, int64_t N, int64_t D,
                       gnnmp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * reduce_nodes(aggr, g, x) / global_pool — GNNlib/src/utils.jl:12-16, GNNlib/src/layers/pool.jl:3-5,
 * for a SORTED graph_indicator (what MLUtils.batch builds, transform.jl:691-699): contiguous segments.
 * seg_ids[N] has values index_base .. index_base+G-1, non-decreasing.  out is [G][D].
 * (An unsorted indicator goes through gnnmp_plan_create(src = 1..N, dst = indicator) + gnnmp_scatter_f32.)
 * One lane group reduces one graph: right for a batch of many small graphs.  For FEW LARGE graphs (a whole-graph
 * readout is G = 1) use the same plan route — it cuts large segments into balanced chunks (N = 2.4 M, G = 1: 283 ms
 * here against 0.3 ms through the plan); the host mirror switches at N > 256 * G.
 * ---------------------------------------------------------------------------------------------- */
int gnnmp_segment_pool_f32(int aggr, const float *x, const void *seg_ids, int idx_bytes,
                           int index_base, float *out, int64_t D, int64_t N, int64_t G,
                           gnnmp_stream_t stream);
/* The same with the segment boundaries precomputed — a constant of the batched graph, like its plan:
 *   gnnmp_segment_bounds   seg_ptr[k] = first node of graph k (k = 0..G; seg_ptr[G] = N), from the sorted indicator, one pass
 *   gnnmp_segment_pool_ptr_f32   the pooling itself: no per-call binary search of the indicator (two 18-step chains of
 *                          dependent loads per graph at N = 245 k: half the kernel's time on the batched config) */
int gnnmp_segment_bounds(const void *seg_ids, int idx_bytes, int index_base, int64_t N, int64_t G, int64_t *seg_ptr,
                         gnnmp_stream_t stream);
int gnnmp_segment_pool_ptr_f32(int aggr, const float *x, const int64_t *seg_ptr, float *out, int64_t D, int64_t N, int64_t G,
                               gnnmp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Dense feature contraction of the layer bodies (the only MFMA work on the path):
 *   out[n][:] = act( W1 * x1[n][:]  (+ W2 * x2[n][:])  (+ bias) )
 * W1 is [Dout][D1], W2 [Dout][D2] row-major (Julia weight' is NOT taken: Julia's (Dout, Din) column-major
 * weight is C row-major [Din][Dout]; pass w_layout = 1 for that, 0 for C row-major [Dout][Din]).
 * Covers `weight * x` (conv.jl:39,69), `weight1*xi .+ weight2*m` (conv.jl:106),
 * `weight * vcat(xi, m)` (conv.jl:281; W1 = first Din columns, W2 = last Din, given by ldw) and
 * `dense_x` (conv.jl:127).  fp32 in, fp32 out.  Round 3: every operand is split EXACTLY into three bf16 planes and the six
 * significant plane products run on v_mfma_f32_32x32x16_bf16 with fp32 accumulation (csrc/msplit.h: error against float64 in the
 * class of an fp32 fma chain, measured lower; non-finite operands are recomputed with fp32 fma loops); shapes whose weight planes
 * do not fit LDS, K % 4 != 0 or Dout % 32 far from full take the fp32 MFMA kernels of rounds 1-2 (v_mfma_f32_16x16x4_f32 /
 * 32x32x2_f32, an exact fp32 fma chain).
 * ldw1/ldw2: leading dimension (elements between consecutive rows of the stored matrix).
 * ---------------------------------------------------------------------------------------------- */
int gnnmp_dense_f32(const float *x1, const float *W1, int64_t D1, int64_t ldw1, const float *x2,
                    const float *W2, int64_t D2, int64_t ldw2, int w_layout, const float *bias,
                    int act, float *out, int64_t N, int64_t Dout, gnnmp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Graph-parallel step for batched graphs (north_star: "shard by graph across up to 8 GPUs of one node with an
 * RCCL-over-xGMI all-gather of per-shard logits").  A batched GNNGraph is block-diagonal (MLUtils.batch,
 * GNNGraphs/src/transform.jl:682-709): member graphs are independent units.  One process per GPU:
 *   1. gnnmp_shard_by_size (HOST arrays): deal the member graphs to the ranks — by decreasing size in a boustrophedon: counts +-1,
 *      node totals within a fraction of a per cent; rank_of[g] = owner, gather_index[g] = row of graph g in the all-gathered block
 *      (rank * gmax + position among the rank's graphs in ascending graph order), *gmax = rows per rank in the collective.
 *   2. every rank batches ITS members (MLUtils.batch), uploads, builds its plan and runs the forward (e.g. gnnmp_graphconv_chain_f32),
 *      writing its (G_r, nout) logits at the start of a (gmax, nout) send buffer (the padding rows are never read back).
 *   3. gnnmp_allgather_f32: ONE ncclAllGather of gmax * nout floats per rank on the caller's communicator and stream (RCCL resolved
 *      with dlopen at the first call; a few KB per rank: latency-bound, no bucketing), then ONE gnnmp_gather_f32 with gather_index
 *      (uploaded once) puts the rows back in graph order.  Weights are replicated; there is no other collective on the path.
 * The host mirror of the same design is gnnmp/parallel.py (torch.distributed, "nccl" = RCCL on ROCm).
 * ---------------------------------------------------------------------------------------------- */
int gnnmp_shard_by_size(const int64_t *sizes, int64_t G, int world, int32_t *rank_of, int64_t *gather_index, int64_t *gmax);
int gnnmp_allgather_f32(void *nccl_comm, const float *send, float *recv, int64_t count, gnnmp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * A whole graph-classification forward in ONE kernel (BASELINE.json config 5):
 *   GNNChain(GraphConv(d0 => d1, σ1; aggr), ..., GraphConv(d_{L-1} => d_L, σL; aggr), GlobalPool(pool_aggr), Dense(d_L => nout))
 *   model: examples/graph_classification_tudataset.jl:79-82; layer body σ.(W1*x_i .+ W2*aggr_j x_j .+ b) GNNlib/src/layers/conv.jl:102-108;
 *   pooling reduce_nodes(aggr, g, x) GNNlib/src/layers/pool.jl:3-5, utils.jl:12-16; head Flux.Dense.
 * on a batched GNNGraph (MLUtils.batch, GNNGraphs/src/transform.jl:682-709): member graphs are contiguous row ranges and no edge
 * crosses them, so a workgroup owns a run of whole graphs and walks the chain without any inter-workgroup traffic; layer outputs
 * live in `scratch` (L2-resident, never read by another workgroup), the last layer is folded straight into per-row head outputs,
 * and only the (G, nout) result is written for the caller.  Contractions run on the split-bf16 MFMA core (fp32-class accuracy).
 *   plan      : plan of the batched graph's (s, t) WITHOUT self loops
 *   seg_ptr   : DEVICE int64 [G + 1], seg_ptr[k] = first node of member graph k (gnnmp_segment_bounds); a member graph may be
 *               empty (seg_ptr[k] == seg_ptr[k + 1]): its row of `out` is b_head (zero without one)
 *   x         : DEVICE [N][d0], 16-byte aligned (both kernels read its rows with 16-byte loads): an x that is not is refused
 *               with GNNMP_EUNSUPPORTED and nothing is written; so is an under-aligned `scratch` whenever the call uses it (the
 *               wave-pair kernel below does not).  Every other array of the call (the weights, the biases, seg_ptr, out) may start
 *               at any multiple of its element size
 *   dims      : HOST int64 [n_layers + 1] = d0 .. dL;  W_root / W_agg / bias : HOST arrays of n_layers DEVICE pointers
 *               (weight1 / weight2; bias entries may be NULL, `bias` itself may be NULL);  act : HOST int [n_layers] (gnnmp_act:
 *               IDENTITY | RELU)
 *   w_layout  : like gnnmp_dense_f32 — 0: every weight is C row-major [out][in]; 1: Julia's (out, in) column-major matrices as stored
 *               (weight1, weight2 and the head's weight alike)
 *   aggr, pool_aggr : GNNMP_SUM | GNNMP_MEAN;  W_head (nout, dL) in the same layout, b_head [nout] or NULL
 *   scratch   : DEVICE, at least gnnmp_graphconv_chain_scratch_floats(N, n_layers, dims, nout) floats, 16-byte aligned
 *   out       : DEVICE [G][nout]
 * Envelope: n_layers <= 4, every d a multiple of 4, d1..dL <= 128, nout <= 8; outside it (or with max / min aggregation) the call
 * returns GNNMP_EUNSUPPORTED without touching `out` and the caller runs the chain layer by layer (gnnmp_propagate_f32 +
 * gnnmp_dense_f32 + gnnmp_segment_pool_ptr_f32).  The pooled-then-Dense order of the reference and the Dense-then-pooled order used
 * here agree to rounding (both are linear); the per-row aggregates have the bits of gnnmp_propagate_f32's.
 * ---------------------------------------------------------------------------------------------- */
int64_t gnnmp_graphconv_chain_scratch_floats(int64_t N, int n_layers, const int64_t *dims, int64_t nout);
/* Optional per-batch constant (like the plan): the member graphs packed into jobs of at most 64 rows (best fit decreasing), which lets
 * the chain 16 => 128 => 128 run with a PAIR OF WAVES per group of whole member graphs and no layer output in memory at all
 * (csrc/graph_chain2.hip: layer 1's accumulators are layer 2's operands, the neighbour sums of layer 2 run after its product through
 * a 4 KB LDS stage the two waves share, the two 64-column halves of layer 2 go to different workgroups; each row's W_head * h2 — nout
 * floats per half — is the only intermediate written, and a second small launch pools it per member graph in node order: no
 * floating-point atomic, no memset, run-to-run identical).  The handle owns that intermediate and the list of jobs set aside for the
 * exact fp32 path (non-finite operands), so — like a plan's workspace — it serves ONE stream at a time.  The list's counter is re-armed on
 * the device by the call's own last launch: nothing about it is chosen on the host, and a recorded call may be replayed back to back.
 * Built once per batched graph from the DEVICE seg_ptr; synchronises `stream` (graph prep).  A batch with a member graph of more than
 * 64 nodes or of none (an empty member), or without any member, yields a handle without jobs: the chain then runs on the general kernel.  info[0] = jobs, [1] = member
 * graphs, [2] = rows, [3] = largest member graph, [4] = per-mille of the MFMA tiles' rows that are real rows. */
typedef struct gnnmp_chain_jobs gnnmp_chain_jobs_t;
int gnnmp_chain_jobs_create(gnnmp_chain_jobs_t **out, const int64_t *seg_ptr, int64_t G, gnnmp_stream_t stream);
int gnnmp_chain_jobs_destroy(gnnmp_chain_jobs_t *jobs);
int gnnmp_chain_jobs_info(const gnnmp_chain_jobs_t *jobs, int64_t *info);
/* The same packing ON THE DEVICE (csrc/chain_pack.h: best fit decreasing on the histogram of the jobs' free room, one thread block): one
 * launch, no copy of the sizes to the host, no synchronisation — the per-step form for a loop that makes a new batch every step
 * (examples/graph_classification_tudataset.jl:97-104).  The caller passes what it holds on the host (num_nodes of every member graph is a
 * host integer, GNNGraphs/src/gnngraph.jl:108-117): n_rows = the batch's nodes, max_graph = its largest member, has_empty = some member has
 * no node.  max_graph > 64 or has_empty gives a handle without jobs, as above.  If the device finds sizes that contradict the announcement
 * the handle is poisoned: the chain writes NaN logits and gnnmp_chain_jobs_info fails.  gnnmp_chain_jobs_info on such a handle
 * synchronises the device.  A jobs handle serves ONE stream at a time and one host thread at a time (its z rows and set-aside list are
 * scratch of the running call).
 *   gnnmp_chain_jobs_release  stream-ordered destroy (see gnnmp_plan_release)
 *   gnnmp_chain_jobs_export   the job table as the kernel reads it: tab_out[cap_rows][64] int32 (global row of each slot, -1 = empty;
 *                             all cap_rows rows are written: a row at or above the job count holds -1 in every slot),
 *                             hdr_out[32] int32 ([0] jobs [1] 32-row tiles [2] poisoned [3] largest member seen [4] empty members,
 *                             [16..29] seven 64-bit phase stamps of the packing kernel, 100 MHz; a handle packed on the host
 *                             (gnnmp_chain_jobs_create) gives [0] jobs, [3] the largest member, [4] 1 if some member is empty, and 0
 *                             in every other word, and the call then synchronises `stream`): tests and tools.  Either output may
 *                             be NULL */
int gnnmp_chain_jobs_pack(gnnmp_chain_jobs_t **out, const int64_t *seg_ptr, int64_t G, int64_t n_rows, int64_t max_graph, int has_empty,
                          gnnmp_stream_t stream);
int gnnmp_chain_jobs_release(gnnmp_chain_jobs_t *jobs, gnnmp_stream_t stream);
int gnnmp_chain_jobs_export(const gnnmp_chain_jobs_t *jobs, int32_t *tab_out, int64_t cap_rows, int32_t *hdr_out, gnnmp_stream_t stream);
/* jobs: NULL or the handle of THIS batch (gnnmp_chain_jobs_create on the same seg_ptr) */
int gnnmp_graphconv_chain_f32(gnnmp_graph_t *plan, const gnnmp_chain_jobs_t *jobs, const int64_t *seg_ptr, int64_t G, const float *x, int n_layers,
                              const int64_t *dims, const float *const *W_root, const float *const *W_agg,
                              const float *const *bias, const int *act, int w_layout, int aggr, int pool_aggr, const float *W_head,
                              const float *b_head, int64_t nout, float *scratch, float *out, gnnmp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Aggregate-then-transform in one kernel — the layer bodies whose dense product FOLLOWS the aggregation:
 *   gcn_conv with Dout >= Din   σ.(W * (cin .* Σ_j w_j cout_j x_j) .+ b)      GNNlib/src/layers/conv.jl:59-71
 *   graph_conv                  σ.(W1 * x_i .+ W2 * aggr_j x_j .+ b)           conv.jl:102-108
 *   sage_conv                   σ.(W * vcat(x_i, aggr_j x_j) .+ b)             conv.jl:277-283
 *     out[i][:] = act( W_root * xi[i][:]  +  W_agg * A[i][:]  + bias ),   A = gnnmp_propagate(_slots)_f32's result
 * with A never written to HBM (it is BIT-IDENTICAL to what gnnmp_propagate_slots_f32 would return; pass agg_out to get it
 * as well, e.g. to test that).  The aggregation arguments mean what they mean in gnnmp_propagate_f32 (w: per-edge weights in
 * original order, scale_src / scale_dst per node) and gnnmp_propagate_slots_f32 (w_slot / ss_slot in plan slot order; they
 * take precedence); scalings need aggr = SUM | MEAN.  xi = NULL / D1 = 0: no root term (gcn_conv).  W_root [Dout][D1] and
 * W_agg [Dout][D] as in gnnmp_dense_f32 (w_layout, ldw).  Shapes taken: D, D1 multiples of 4 and <= 128, Dout a multiple of
 * 4 and <= 128, 16-byte aligned arrays, >= 16 destinations; anything else returns GNNMP_EUNSUPPORTED and the caller runs
 * gnnmp_propagate_f32 + gnnmp_dense_f32.  One stream at a time per plan (plan-owned workspace and tile ticket).
 * ---------------------------------------------------------------------------------------------- */
int gnnmp_fused_conv_f32(gnnmp_graph_t *plan, int aggr, const float *xj, const float *w, const float *scale_src,
                         const float *w_slot, const float *ss_slot, const float *scale_dst, int64_t D, const float *xi,
                         int64_t D1, const float *W_root, int64_t ldw_root, const float *W_agg, int64_t ldw_agg,
                         int w_layout, const float *bias, int act, float *out, int64_t Dout, float *agg_out,
                         gnnmp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Adjoints.  The reference trains through NNlib's rrules: ∇gather = scatter(+),
 * ∇scatter(+) = gather, ∇scatter(mean) = gather ./ count, ∇scatter(max|min) = (src .== gather(dst)) .* gather(Δ);
 * the CPU fast path through the adjacency_matrix rrule (GNNGraphs/src/query.jl:244-278).
 *
 * The adjoint of the fused propagate w.r.t. xj needs no entry point of its own: build a plan of the TRANSPOSED edge
 * index (gnnmp_plan_create(..., src = t, dst = s, ...)) and call
 *   gnnmp_propagate_f32(plan_T, msg, GNNMP_SUM, Δ, w, scale_src = scale_dst_fwd (./ count for MEAN), scale_dst = scale_src_fwd, Δx, D)
 * (same per-source edge order as NNlib's scatter(+, gather(Δ, t) .* w, s)).  The two that do:
 * ---------------------------------------------------------------------------------------------- */
/* out[k] = Σ_d a_dst[dst_k][d] * b_src[src_k][d] for every edge k (original order) — the adjoint w.r.t. the edge
 * weights of w_mul_xj / e_mul_xj:  Δw = sum(Δm .* xj_gathered, dims = 1)  with Δm = gather(Δ, t). */
int gnnmp_edge_dot_f32(const float *a_dst, const float *b_src, const void *src, const void *dst,
                       int idx_bytes, int index_base, int64_t n_edges, int64_t D, float *out,
                       gnnmp_stream_t stream);
/* The same per-edge dot products walked in the plan's destination-sorted order (the destination row stays in registers
 * for all of its edges: half the traffic); out[n_edges] is written in ORIGINAL edge order, plan-added self loops
 * produce no output.  The row must fit one wave of the widest lanes D and the two feature pointers admit — 16-byte lanes (D <= 256) when
 * D % 4 == 0 and a_dst, b_src are 16-byte aligned, 8-byte lanes (D <= 128) when D % 2 == 0 and both are 8-byte aligned, 4-byte lanes
 * (D <= 64) otherwise — else GNNMP_EUNSUPPORTED (gnnmp_edge_dot_f32 takes any D and any float-aligned pointer). */
int gnnmp_edge_dot_plan_f32(gnnmp_graph_t *plan, const float *a_dst, const float *b_src, float *out,
                            int64_t D, gnnmp_stream_t stream);
/* Adjoint of propagate(copy_xj, g, max|min) w.r.t. xj on the transposed plan:
 *   Δx_j[d] = Σ_{k: s_k = j, edge order} (x_j[d] == y_{t_k}[d]) ? Δ_{t_k}[d] : 0      (ties all receive Δ, like NNlib)
 * x: forward input [n][D], y: forward output, dy: incoming gradient, dx: output. */
int gnnmp_propagate_maxmin_grad_f32(gnnmp_graph_t *plan_transposed, const float *x, const float *y,
                                    const float *dy, float *dx, int64_t D, gnnmp_stream_t stream);

/* Adjoints of the dense part  y = σ.(W * x .+ b):
 *   gnnmp_act_grad_f32      Δz = Δy .* σ'(z)  (relu: Δy where y > 0, else 0; identity: copy).  dz may alias dy.
 *   gnnmp_dense_grad_w_f32  ΔW[o][k] = Σ_n Δz[n][o] x[n][k]  ([Dout][K] row-major) and/or Δb[o] = Σ_n Δz[n][o]
 *                           (either output may be NULL); fp32 MFMA, operands read straight from HBM, per-slab partials in
 *                           `workspace` (gnnmp_dense_grad_workspace(N, Dout, K) floats) folded in slab order: no atomics.
 *   Δx = W' * Δz is the forward kernel: gnnmp_dense_f32(Δz, W, D1 = Dout, ldw1 = K, ..., w_layout = 1, ..., Dout = K). */
int gnnmp_act_grad_f32(const float *dy, const float *y, int act, float *dz, int64_t n, gnnmp_stream_t stream);
/* The training step of the graph-classification chain (examples/graph_classification_tudataset.jl:79-82,97-104) with fewer passes over
 * the (N, D) arrays — the same arithmetic as the entry points above, fused where two of them touched one array (round 5):
 *   gnnmp_dense_grad_w2_f32   ΔW1 = Δz' x1, ΔW2 = Δz' x2 and Δb = colsum(Δz) from ONE read of Δz — graph_conv's / sage_conv's two weight
 *                             gradients (conv.jl:102-108: x1 = x_i, x2 = the aggregate).  out = [ΔW1 (Dout x K1) | ΔW2 (Dout x K2) | Δb
 *                             (Dout)], contiguous; K1 a multiple of 16 (else GNNMP_EUNSUPPORTED: call gnnmp_dense_grad_w_f32 twice);
 *                             workspace: gnnmp_dense_grad_w2_workspace floats.  Same slabs, same fold order: the three results are
 *                             bit-identical to the separate calls.
 *   gnnmp_pool_grad_act_f32   dz[i][:] = act'(y[i][:]) .* dpool[g(i)][:] (.* inv_count[g(i)] if given): the pullback of
 *                             reduce_nodes(+ | mean) (utils.jl:12-16, NNlib's ∇scatter = gather) and of the activation of the layer
 *                             that fed the pool, one pass instead of mul_rows + gather + act_grad.
 *   gnnmp_propagate_add_mask_f32   out[i][:] = act'(mask_y[i][:]) .* (addend[i][:] + Σ_{j -> i} xj[j][:]) — the x-pullback of graph_conv,
 *                             Δx = Δz W_root + Aᵀ(Δz W_agg), with the sum and the relu' of the layer below in the row kernel's
 *                             epilogue (plan = the plan of the REVERSED edges; aggr + or mean with scale_dst = 1 / count as in
 *                             gnnmp_propagate_f32; addend / mask_y optional). */
int64_t gnnmp_dense_grad_w2_workspace(int64_t N, int64_t Dout, int64_t K1, int64_t K2);
int gnnmp_dense_grad_w2_f32(const float *dz, const float *x1, int64_t K1, const float *x2, int64_t K2, int64_t N, int64_t Dout,
                            float *out, float *workspace, int64_t workspace_floats, gnnmp_stream_t stream);
int gnnmp_pool_grad_act_f32(const float *dpool, const void *graph_indicator, int idx_bytes, int index_base, const float *inv_count,
                            const float *y, int act, float *dz, int64_t N, int64_t G, int64_t D, gnnmp_stream_t stream);
int gnnmp_propagate_add_mask_f32(gnnmp_graph_t *plan, int aggr, const float *xj, const float *scale_dst, const float *addend,
                                 const float *mask_y, float *out, int64_t D, gnnmp_stream_t stream);
int64_t gnnmp_dense_grad_workspace(int64_t N, int64_t Dout, int64_t K);
int gnnmp_dense_grad_w_f32(const float *dz, const float *x, int64_t N, int64_t Dout, int64_t K, float *dW,
                           float *db, float *workspace, int64_t workspace_floats, gnnmp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * TGCN's recurrence (GraphNeuralNetworks/src/layers/temporalconv.jl:809-849 TGCNCell, scanned over time by GNNRecurrence :121-135).
 * The cell's three graph convolutions depend on x_t only, so the caller computes them for all T steps up front and passes the input
 * halves of the three Dense layers, P[n][t] = (W_z[:, 1:out] conv_z + b_z, W_r[:, 1:out] conv_r + b_r, W_h[:, 1:out] conv_h + b_h),
 * [N][T][3 out].  What remains per step is node-local (U_g = W_g[:, out+1:2out], the state half of dense_g):
 *   z = σ(P_z + U_z h), r = σ(P_r + U_r h), h~ = tanh(P_h + U_h (r .* h)), h' = (1 - z) .* h + z .* h~     (:840-849)
 *   gnnmp_tgcn_recurrence_f32       all T steps in ONE launch, 16 nodes a wave, the state in registers, U in LDS, fp32 MFMA.
 *                                   U_zr [2 out][out] = (U_z; U_r), U_h [out][out], row-major.  h0: [N][out] (h0_stride = out), one
 *                                   vector for every node (h0_stride = 0) or NULL (zeros: initialstates).  y [N][T][out]; gates
 *                                   [N][T][3 out] = (z, r, h~) for the pullback, or NULL.  1 <= out <= 128, else GNNMP_EINVAL.
 *   gnnmp_tgcn_recurrence_grad_f32  the reverse-time pullback in ONE launch, given dy [N][T][out] and the forward's y / gates / h0:
 *                                   dP [N][T][3 out] (the pre-activation gate gradients = ΔP), S [N][T][2 out] = (h_{t-1}, r .* h_{t-1})
 *                                   (nullable: the operands of ΔU_zr = ΔP_zr' h_{t-1}, ΔU_h = ΔP_h' (r .* h_{t-1}) over N T rows, e.g.
 *                                   gnnmp_dense_grad_w_f32), dh0 [N][out] (nullable).
 * No atomics: every output element is written by one lane, run-to-run identical.  The per-step halves of the same arithmetic (any out;
 * the caller runs U's products per step with gnnmp_dense_f32, t = the step, arrays as above, a / drh / part / dah / dzr contiguous):
 *   gnnmp_tgcn_step_f32       phase 0: z, r = σ(P_zr[t] + a) -> gates[t], hout = r .* h;  a = h U_zr' [N][2D]
 *                             phase 1: h~ = tanh(P_h[t] + a) -> gates[t], h' -> y[t] and hout;  a = (r .* h) U_h' [N][D]
 *                             h: the state (row stride ldh; NULL = zeros)
 *   gnnmp_tgcn_step_grad_f32  phase 0: Δh = dy[t] + carry (nullable); ΔP_z, ΔP_h -> dP[t], dah = ΔP_h, dzr[:, 0:D] = ΔP_z, part = Δh (1 - z)
 *                             phase 1: drh = ΔP_h U_h; ΔP_r -> dP[t], dzr[:, D:2D]; part += drh .* r; S[t] (nullable)
 *                             (then carry = part + dzr U_zr for step t - 1) */
int gnnmp_tgcn_recurrence_f32(const float *P, const float *U_zr, const float *U_h, const float *h0, int64_t h0_stride, float *y,
                              float *gates, int64_t N, int64_t T, int64_t out, gnnmp_stream_t stream);
int gnnmp_tgcn_recurrence_grad_f32(const float *dy, const float *y, const float *gates, const float *U_zr, const float *U_h,
                                   const float *h0, int64_t h0_stride, float *dP, float *S, float *dh0, int64_t N, int64_t T,
                                   int64_t out, gnnmp_stream_t stream);
int gnnmp_tgcn_step_f32(int phase, const float *P, const float *a, const float *h, int64_t ldh, float *gates, float *hout, float *y,
                        int64_t N, int64_t T, int64_t t, int64_t D, gnnmp_stream_t stream);
int gnnmp_tgcn_step_grad_f32(int phase, const float *dy, const float *carry, const float *gates, const float *h, int64_t ldh,
                             const float *drh, float *dP, float *dah, float *dzr, float *part, float *S, int64_t N, int64_t T, int64_t t,
                             int64_t D, gnnmp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Link prediction (GraphNeuralNetworks/examples/link_prediction_pubmed.jl).  The reference runs both graph transforms on the CPU
 * (edge_index copied to the host and back); here they stay on the device.  Random draws are counter based: the same seed gives the
 * same result, but it is NOT Julia's RNG stream, so parity with the reference is distributional.  Indices keep the input's width and
 * base.  Integers only at the seam: the reference's Float64 formulas are evaluated inside.
 *
 *   gnnmp_negative_sample   negative_sample(g; num_neg_edges, bidirected, max_trials) — GNNGraphs/src/transform.jl:890-929.
 *                           Positives: g's n_edges edges plus a self loop on every node (E' = n_edges + n_nodes); codes
 *                           (s-1) n + t, maxid = n^2.  bidirected: num_neg_edges / 2 first.  pneg = 1 - E' / (2 maxid),
 *                           p = min(1, num_neg / (pneg maxid) * 1.1) (pneg = 0: p = 1; n_nodes = 0: nothing to draw, no edges);
 *                           p < 0 or num_neg_edges < 0: GNNMP_EINVAL.  Each of up to max_trials trials draws randsubseq(1:maxid, p)
 *                           (ascending), drops the positives and the codes kept so far, appends the rest; once num_neg codes are kept
 *                           the list is cut to its first num_neg (the last trial's LOWEST codes) and the trials stop.  Writes the
 *                           decoded pairs, followed by the swapped pairs when bidirected, to s_out / t_out; *total (host) = edges
 *                           written, possibly fewer than asked for (as in the reference) when the trials run out.  capacity >=
 *                           (bidirected ? 2 (num_neg_edges / 2) : num_neg_edges), else GNNMP_EINVAL.  Work and memory
 *                           O(n_edges + candidates), never O(n^2): the code space is cut into chunks walked by geometric gaps, the
 *                           positives sorted once (device radix sort).  Synchronisations: 1 (the positives' sort) + 1 per trial (its
 *                           kept count), + 1 per further trial (the sort of the codes kept so far); the outputs are complete on return.
 *   gnnmp_rand_edge_split   rand_edge_split(g, frac; bidirected) — GNNGraphs/src/transform.jl:945-968.  ne = bidirected ? n_edges / 2 :
 *                           n_edges; size1 = round(ne frac) (computed by the caller: round half to even); eids = a uniformly random
 *                           permutation of 1:ne (radix sort of counter-based keys).  Not bidirected: part 1 = edges eids[1:size1] in
 *                           permutation order, part 2 the rest.  Bidirected: the edges with s < t, compacted in edge order, are
 *                           indexed instead, and each part is written as [s; t], [t; s] — s1 / t1 hold 2 size1 entries, s2 / t2
 *                           2 (ne - size1).  Fewer than ne edges with s < t: GNNMP_EBOUNDS (the reference's BoundsError).
 *                           Synchronisations: 1 (the permutation's sort) + 1 when bidirected.
 *   gnnmp_edge_dot_grad_f32 the adjoint of z_k = <xi[t_k], xj[s_k]> (apply_edges(xi_dot_xj, g, xi, xj), GNNlib/src/msgpass.jl:172;
 *                           DotDecoder, GNNlib/src/layers/basic.jl:1-3) w.r.t. the node features, given dz[n_edges] in original edge
 *                           order:  dxi[v] = Σ_{k: t_k = v} dz_k xj[s_k]  (walks the plan's row v),  dxj[u] = Σ_{k: s_k = u} dz_k
 *                           xi[t_k]  (the transposed plan's row u), in edge order, each row summed in registers and written once: no
 *                           atomics, reruns are bit-identical.  Alias mode, dxi == dxj (requires xi == xj): dx[v] = (in-edge sum) +
 *                           (out-edge sum), one launch.  Either output may be NULL in split mode.  Plans without added self loops
 *                           (else GNNMP_EINVAL); D <= 256, else GNNMP_EUNSUPPORTED (compose two w_mul_xj propagates with w = dz).
 * ---------------------------------------------------------------------------------------------- */
int gnnmp_negative_sample(const void *s, const void *t, int idx_bytes, int index_base, int64_t n_edges, int64_t n_nodes,
                          int64_t num_neg_edges, int bidirected, int max_trials, uint64_t seed, void *s_out, void *t_out,
                          int64_t capacity, int64_t *total, gnnmp_stream_t stream);
int gnnmp_rand_edge_split(const void *s, const void *t, int idx_bytes, int index_base, int64_t n_edges, int bidirected, int64_t size1,
                          uint64_t seed, void *s1, void *t1, void *s2, void *t2, gnnmp_stream_t stream);
int gnnmp_edge_dot_grad_f32(gnnmp_graph_t *plan, gnnmp_graph_t *plan_transposed, const float *xi, const float *xj, const float *dz,
                            float *dxi, float *dxj, int64_t D, gnnmp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Neighbour search (csrc/neighbors.hip): the graph constructors knn_graph(points, k; graph_indicator, self_loops, dir) and
 * radius_graph(points, r; ...) — GNNGraphs/src/generate.jl:112-145, 196-222.  The reference runs NearestNeighbors.jl trees on the
 * CPU; here an exact brute-force search in fp32 on the device.  points: [N][d] row-major (Julia's d x N), 4-byte aligned.
 *
 * Fixed semantics (the answer is unique and does not depend on tiling; reruns are bit-identical):
 *   - d2(i, j) is accumulated over the dimensions c = 0 .. d-1 in order from 0 as acc = fmaf(x[i][c] - x[j][c], x[i][c] - x[j][c], acc);
 *     a non-finite d2 (NaN included) ranks as +inf.
 *   - candidates are ordered by the pair (d2, j): ties go to the lower index.
 *   - graph_indicator (nullable; idx_bytes 4 | 8, values index_base .. index_base + n_graphs - 1; both ignored without it): the
 *     candidates of i are the nodes with i's graph id, on the RAW coordinates (the reference rescales the points and appends a dummy
 *     coordinate, generate.jl:125-130).  Non-decreasing indicator: the candidate range is the graph's segment (gnnmp_segment_bounds),
 *     work sum n_g^2; otherwise the full range with the other graphs masked.  An id outside the n_graphs graphs: GNNMP_EBOUNDS.
 *   - self_loops = 0 excludes j == i BY INDEX (a duplicated point is a neighbour at distance 0); != 0: i is a candidate like any other.
 *
 * The result is a PLAN, like gnnmp_plan_concat / gnnmp_plan_select hand out graphs: the reference's adjacency list -> COO conversion
 * (convert.jl:97-117) numbers the edges centre by centre, so the edge list is destination-sorted as it is produced and the kernels
 * write the plan's arrays themselves — row i = centre i, its slots = i's neighbours, eid[e] = e — with no sort and no copy (what
 * gnnmp_plan_from_csc(colptr, rowval) would build).  *out is owned by the caller (gnnmp_plan_destroy), n_src = n_dst = N, no self loops
 * added.  The edge list in any index width and base: gnnmp_plan_edge_index(plan, idx_bytes, index_base, s, t) gives dir = :in
 * (s = neighbour, t = centre); pass the two output pointers swapped for dir = :out, for which this plan is the plan of the REVERSED
 * edges (t, s).  rowptr / degrees: gnnmp_plan_export64; the number of edges: gnnmp_plan_info.
 *
 *   gnnmp_knn_graph_f32     N k edges: edge i k + r joins centre i and its r-th nearest candidate, r in rank order.  1 <= k <= 1024
 *                           (k > 64 runs ceil(k / 64) passes over the candidates).  A graph that occurs in the indicator with fewer
 *                           than k (k + 1 without self loops) nodes — or N below that without an indicator — is GNNMP_EBOUNDS before the
 *                           launch (the reference's @assert all(values(cm) .>= k)).
 *   gnnmp_radius_graph_f32  j is a neighbour of i iff d2(i, j) <= r2, r2 = r * r formed once in fp32 (r >= 0; r < 0 or NaN:
 *                           GNNMP_EINVAL).  Centres ascend, the neighbours of a centre ascend in j.  A count pass, an exclusive scan
 *                           (the total is read on the host: it sizes the plan) and a write pass.
 * Both synchronise the stream, as every plan build does (+ once for an indicator's checks, twice when it is unsorted).  Arguments are
 * checked before any HIP call.  Workspace: the segment table, the scan's scratch and int64[N + 1]; no N x N or N x tile array exists
 * in memory.  No atomics in the search kernels (the graph sizes of an UNSORTED indicator are counted with integer adds).
 * N < 2^31 - 1, d <= 2^20, edges < GNNMP_MAX_SLOTS.
 *
 *   gnnmp_hyperbolic_graph_f32  the radius search in the hyperbolic plane: the N x N loop of rand_temporal_hyperbolic_graph
 *                           (generate.jl:287-297, 359-369).  points: [N][2] = (r, theta), r >= 0, any real theta (no wrap is needed or
 *                           done).  j is a neighbour of i iff the hyperbolic distance at curvature parameter zeta is at most R:
 *                           acosh(cosh zeta r_i cosh zeta r_j - sinh zeta r_i sinh zeta r_j cos(theta_i - theta_j)) / zeta <= R, evaluated
 *                           as v(i, j) <= cosh(zeta R) (acosh is monotone) in the cancellation-free form
 *                               v = cosh(zeta (r_i - r_j)) + 2 sinh zeta r_i sinh zeta r_j sin^2((theta_i - theta_j) / 2)
 *                                 = ((E_i F_j + F_i E_j) + S_i S_j h) / 2,   E = e^(zeta r), F = e^(-zeta r), S = sinh(zeta r),
 *                                   h = (cos theta_i - cos theta_j)^2 + (sin theta_i - sin theta_j)^2.
 *                           E, F, S are computed per node in double and rounded to fp32 once; cos theta and sin theta stay in double
 *                           and h is rounded to fp32 once (an fp32 difference of two angles across the 0 / 2 pi seam would have lost
 *                           the digits that count); the rest is fp32: t = fmaf(F_i, E_j, E_i F_j) (t = 2 exactly when E_i == E_j),
 *                           2 v = t + (S_i S_j) h, compared with fl32(2 cosh(zeta R)) formed in double.  No transcendental per pair.
 *                           Error, with u = 2^-24, against the exact v of the fp32 inputs (points, R, zeta as passed):
 *                               |v_dev - v| <= 6 u v + S_i S_j 2^-50 sqrt(h),   and the threshold carries one more u:
 *                           the answer is the exact one for every pair with |v - cosh(zeta R)| > 8 u cosh(zeta R), the second term being
 *                           below u v when sqrt(h) >= 2^-25 or zeta (r_i + r_j) <= 36 (S_i S_j <= e^36 / 4).  tests/temporal_gen_ref.py
 *                           holds the same bound as B = 8.
 *                           self_loops != 0: every node with finite (r, theta) gets its loop (v = 1 by definition, not computed);
 *                           == 0: j == i is skipped by index.  Distinct nodes at identical coordinates are joined (v = 1 exactly).
 *                           A pair whose value is not finite is no edge: a node with NaN or infinite r or theta has none; every value
 *                           is finite while zeta r <= 44 for all nodes; above, a pair with zeta (r_i + r_j) > 88 may overflow, and a
 *                           node with zeta r > 88.7 (E = +inf) has no edge but its loop.  A negative r evaluates the same formula, with
 *                           cancellation (the bound above does not hold).  R < 0 or NaN, zeta <= 0 or not finite: GNNMP_EINVAL, as is
 *                           everything gnnmp_radius_graph_f32 refuses; zeta R > 88.7 makes the threshold +inf (every finite pair).
 *                           Shape, order, indicator handling and synchronisations are gnnmp_radius_graph_f32's: a count pass, the scan
 *                           (total read on the host), a write pass; centres ascend, the neighbours of a centre ascend in j; no atomics,
 *                           reruns are bit-identical.  One launch more (the per-node pre-pass) and 32 N bytes more workspace.
 * ---------------------------------------------------------------------------------------------- */
int gnnmp_hyperbolic_graph_f32(gnnmp_graph_t **out, const float *points, int64_t N, float R, float zeta, const void *graph_indicator,
                               int idx_bytes, int index_base, int64_t n_graphs, int self_loops, gnnmp_stream_t stream);
int gnnmp_knn_graph_f32(gnnmp_graph_t **out, const float *points, int64_t N, int64_t d, int64_t k, const void *graph_indicator,
                        int idx_bytes, int index_base, int64_t n_graphs, int self_loops, gnnmp_stream_t stream);
int gnnmp_radius_graph_f32(gnnmp_graph_t **out, const float *points, int64_t N, int64_t d, float r, const void *graph_indicator,
                           int idx_bytes, int index_base, int64_t n_graphs, int self_loops, gnnmp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Heterogeneous graphs: the aggregation of one layer over typed relations in ONE launch (csrc/hetero.hip).  HeteroGraphConv
 * (GraphNeuralNetworks/src/layers/heteroconv.jl:57-86) applies one layer per relation (src_type, rel, dst_type) and folds the outputs per
 * destination type, foldl(aggr, outs).  For every destination type d of the call and every row i < n_dst:
 *     out_d[i][:] = foldl(combine_d, m_1[i], ..., m_R[i]),     m_r = what gnnmp_propagate_f32(plan_r, msg, aggr_r, x_r, w_r) returns
 * (msg = W_MUL_XJ where w_r is given, else COPY_XJ; no scale vectors), relations in table order, the m_r never written: a lane group
 * walks row i in each relation in turn, in ORIGINAL edge order, and keeps the running value in registers.  An empty row contributes the
 * operator's identity (0 / 0 / -Inf / +Inf), MEAN divides by the row's count, exactly as gnnmp_propagate_f32 does.
 *   gnnmp_hetero_rel_t  plan: the relation's plan (n_dst = the destination type's), x [n_src][D], w [n_edges] in original edge order or
 *                       NULL, aggr: its own gnnmp_aggr.  plan = NULL is an IDENTITY relation: it contributes row i of x [n_dst][D] as
 *                       it is (w is ignored; aggr must still be a gnnmp_aggr) — a layer's root term, or finished layer outputs to be combined.
 *   gnnmp_hetero_dst_t  out [n_dst][D], combine: GNNMP_SUM | GNNMP_MAX | GNNMP_MIN (Base.max / Base.min as everywhere), n_rel >= 1 records.
 * `dsts` and every `rels` are HOST arrays (the grouped-call form of gnnmp_graphconv_chain_f32's host tables of device pointers); out, x and
 * w are device pointers.  The tables travel by value in the kernel arguments: the call neither allocates nor synchronises, uses no
 * plan-owned scratch (plans are only read: two streams may share one), and may be recorded into a HIP graph without an eager call first.
 * Refused before any HIP call: GNNMP_EINVAL for a NULL or empty table, D outside 1 .. 2^20, a NULL out / x that would be dereferenced,
 * a bad combine / aggr, a plan whose n_dst is not the record's; GNNMP_EUNSUPPORTED for more than GNNMP_HETERO_MAX_REL relations in one
 * call (all destination types together).  Rows of at most the plan's long-row threshold are bit-identical to the per-relation calls
 * folded in order; a longer row is walked whole, in edge order (bit-identical to the sequential loop, slow for hubs — a caller with
 * split rows composes gnnmp_propagate_f32 per relation and combines with identity relations).
 * ---------------------------------------------------------------------------------------------- */
#define GNNMP_HETERO_MAX_REL 16
typedef struct {
    const gnnmp_graph_t *plan;
    const float *x;
    const float *w;
    int aggr;
} gnnmp_hetero_rel_t;
typedef struct {
    float *out;
    int64_t n_dst;
    int combine;
    int n_rel;
    const gnnmp_hetero_rel_t *rels;
} gnnmp_hetero_dst_t;
int gnnmp_hetero_propagate_f32(const gnnmp_hetero_dst_t *dsts, int n_dsts, int64_t D, gnnmp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * The adjoint of the heterograph aggregation w.r.t. the node features, in ONE launch over all source types (csrc/hetero_backward.hip):
 * the forward's shape, mirrored.  For every source type S of the call and every row j < n_src:
 *     dx_S[j][:] = c_1[j] + ... + c_R[j]        (table order; the first term is copied, not added to zero)
 * a lane group owns row j, walks it in each outgoing relation's TRANSPOSED plan (a plan built from (t, s): rows = source nodes, col =
 * destination, slots in ORIGINAL edge order) and keeps the running sum in registers: no per-relation [n_src][D] matrix is written.
 * Each record takes one of four modes:
 *   linear           plan_t given, y NULL — the adjoint of + / mean, with or without edge weights:
 *                    c[j] = sum over the slots p of row j, in edge order, of w[eid_p] * (dy[col_p] * sd[col_p]), every product rounded, sd
 *                    first (the order of gnnmp_propagate_f32 with scale_src = sd); an absent w or sd is 1.0f.  mean: sd = 1 / count.
 *   winners          plan_t and y given — the adjoint of max / min over copy_xj (NNlib: every tie receives the gradient):
 *                    c[j][f] = sum over the slots p of row j of (x_S[j][f] == y[col_p][f] ? dy[col_p][f] : 0).  w or sd: GNNMP_EINVAL.
 *   identity         plan_t NULL, y and out NULL — c[j] = dy[j] (dy is [n_src][D]): a layer's root term, a type that is its own source.
 *   masked identity  plan_t NULL, y and out given ([n_src][D] each) — c[j][f] = (y[j][f] == out[j][f]) ? dy[j][f] : 0: the pullback of ONE
 *                    term y of out = foldl(max | min, terms).  EVERY term that ties with the result receives the gradient.  That tie rule is
 *                    this project's own, chosen to agree with the winners mode; how the reference's AD splits a tie of a fold of `max` is
 *                    not pinned anywhere here (ties have measure zero for real-valued features).
 *   gnnmp_hetero_rel_grad_t  plan_t, dy [n_dst][D] (identity: [n_src][D]), w [n_edges] original edge order or NULL, sd [n_dst] a factor per
 *                            GATHERED row or NULL, y [n_dst][D] the relation's forward aggregate (identity: the term that entered the
 *                            fold) or NULL, out [n_src][D] the fold's result (identity relations only) or NULL.
 *   gnnmp_hetero_src_t       dx [n_src][D] (written in full), x [n_src][D] the forward input (read by winners records only; may be NULL
 *                            without one), n_rel >= 1 records.
 * `srcs` and every `rels` are HOST arrays; dx, x, dy, w, sd, y and out are device pointers.  As gnnmp_hetero_propagate_f32: the tables
 * travel by value in the kernel arguments, the call neither allocates nor synchronises, uses no plan-owned scratch (plans are only read)
 * and may be recorded into a HIP graph without an eager call first; a call whose n_src are all 0 launches nothing.  Refused before any
 * HIP call: GNNMP_EINVAL for a NULL or empty table, D outside 1 .. 2^20, a NULL dx / x / dy that would be dereferenced, y together with w
 * or sd, out without y (or with a plan), an identity record with y but no out, a plan whose height is not n_src; GNNMP_EUNSUPPORTED for
 * more than GNNMP_HETERO_MAX_REL records in one call (all source types together).  A row longer than the plan's long-row threshold is
 * walked whole, in edge order (slow for hubs — a caller with split rows composes gnnmp_propagate_f32 on the transposed plan /
 * gnnmp_propagate_maxmin_grad_f32 per relation and sums with the forward export's identity relations).
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
    const gnnmp_graph_t *plan_t;
    const float *dy;
    const float *w;
    const float *sd;
    const float *y;
    const float *out;
} gnnmp_hetero_rel_grad_t;
typedef struct {
    float *dx;
    const float *x;
    int64_t n_src;
    int n_rel;
    const gnnmp_hetero_rel_grad_t *rels;
} gnnmp_hetero_src_t;
int gnnmp_hetero_propagate_grad_f32(const gnnmp_hetero_src_t *srcs, int n_srcs, int64_t D, gnnmp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Heterograph attention: GATConv / GATv2Conv members of a HeteroGraphConv in ONE launch (csrc/hetero_attn.hip) — what
 * GraphNeuralNetworks/src/layers/heteroconv.jl:57-86 composes from gat_conv / gatv2_conv on a relation through expand_srcdst
 * (GNNlib/src/layers/conv.jl:112-214).  For every destination type d of the call and every row i < n_dst:
 *     out_d[i]     = foldl(combine_d, term_1[i], ..., term_R[i])         table order; the first term is copied, not folded into a zero
 *     term_r[i]    = act_r(o_r[i] + bias_r)
 *     o_r[i][h]    = sum_j softmax_{j in N_r(i)}(l_ij[h]) K_j[h]
 *     l_ij[h]      = GNNMP_ATTN_GAT:   leakyrelu(a[h][0:C] . Q_i[h] + a[h][C:2C] . K_j[h])
 *                    GNNMP_ATTN_GATV2: sum_c a[h][c] leakyrelu(Q_ic + K_jc)                 (the logits of gnnmp_attn_conv_f32)
 * A row without an in-edge in relation r has o_r = 0 and statistics (-Inf, 0), as gnnmp_attn_conv_edge_f32 documents.  A lane group owns
 * one destination row: per relation it walks the row whole with an online softmax, finishes term_r in registers, writes stats_r if asked,
 * folds into the running value and stores the row once after the last relation; the terms are never written.
 *   gnnmp_hetero_attn_rel_t  plan: the relation's plan (n_dst = the record's; built without self loops), or NULL = an IDENTITY relation that
 *                            contributes row i of K [n_dst][H*C] as it is (mode, Q, a, bias, stats, act are then ignored, act must still be
 *                            valid).  mode: GNNMP_ATTN_GAT | GNNMP_ATTN_GATV2.  Q [n_dst][H*C] (GAT: Wx_dst; GATV2: dense_i(x_dst)),
 *                            K [n_src][H*C] (GAT: Wx_src; GATV2: dense_j(x_src); also the value), a: GAT [H][2C] (target half first),
 *                            GATV2 [H][C]; bias [H*C] or NULL; stats [n_dst][H][2] = (m_i, den_i) as gnnmp_gat_conv_stats_f32 writes them,
 *                            or NULL; act: GNNMP_ACT_IDENTITY | GNNMP_ACT_RELU.
 *   gnnmp_hetero_attn_dst_t  out [n_dst][H*C], combine: GNNMP_SUM | GNNMP_MAX | GNNMP_MIN, n_rel >= 1 records.
 * `dsts` and every `rels` are HOST arrays; the tables travel by value in the kernel arguments.  The call neither allocates nor
 * synchronises, uses no atomics and no plan-owned scratch (plans are only read), may be recorded into a HIP graph without an eager call
 * first, and two calls give equal bits.  The feature row must fit one wave under the rule of gnnmp_gat_conv_stats_f32: out and every Q
 * and K of the call are the [.][H*C] arrays whose alignment selects v.  An R-relation call has the bits of the R single-relation calls
 * folded in table order with one fp32 + / max / min each.  A row longer than the plan's long-row threshold is walked whole by its lane
 * group: correct, slow (a caller with split rows runs the relations one by one).
 * Refused before any HIP call: GNNMP_EINVAL for a NULL or empty table, H or C < 1, a bad combine / mode / act, a NULL pointer that would
 * be dereferenced, a plan whose n_dst is not the record's, a plan with self loops of its own; GNNMP_EUNSUPPORTED for more than
 * GNNMP_HETERO_MAX_REL records in one call (all destination types together) and for a feature row that does not fit one wave at the v
 * the pointers allow.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
    const gnnmp_graph_t *plan;
    int mode;
    const float *Q;
    const float *K;
    const float *a;
    const float *bias;
    float *stats;
    float negative_slope;
    int act;
} gnnmp_hetero_attn_rel_t;
typedef struct {
    float *out;
    int64_t n_dst;
    int combine;
    int n_rel;
    const gnnmp_hetero_attn_rel_t *rels;
} gnnmp_hetero_attn_dst_t;
int gnnmp_hetero_attn_f32(const gnnmp_hetero_attn_dst_t *dsts, int n_dsts, int64_t H, int64_t C, gnnmp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * EdgeConv with a one-layer nn, forward and pullback — edge_conv, GNNlib/src/layers/conv.jl:237-246:
 *   propagate(edge_conv_message, g, l.aggr; xi = x, xj = x),  edge_conv_message(l, xi, xj, e) = l.nn(vcat(xi, xj .- xi))
 * For nn = Dense(2D => C, σ) with W = [W1 | W2]:  nn(vcat(xi, xj - xi)) = σ(W1 xi + b - W2 xi + W2 xj), so the contraction is ONE dense
 * call of the caller on N rows (gnnmp_dense_f32): P = x [W1; W2]' + [b; 0], and the two exports below do the per-edge rest as passes of a
 * row kernel over gathered rows of P (csrc/edge_conv.hip).  Nothing of E rows is read or written.
 *
 * P is [N][2C] row-major, PLANAR: columns [0, C) are the x_i share with the bias folded in, columns [C, 2C) the x_j share (planar, not
 * interleaved: the per-edge gather fetches only the x_j share).
 *
 * Forward, for destination i and its slots in the plan's order (the original edge order), per channel c:
 *   a_i[c]   = P[i][c] − P[i][C+c]          one rounded subtraction, once per row, kept in registers
 *   pre_e[c] = a_i[c] + P[j][C+c]           one rounded add, no contraction
 *   m_e[c]   = σ(pre_e[c])                  σ ∈ {identity, relu}
 *   y_i[c]   = aggr_e m_e[c]                +, mean (sum / count, true division), max, min
 * The fold is sequential in edge order.  Empty rows keep the identity: 0 / 0 / −Inf / +Inf, as everywhere else in the ABI.
 *
 * Backward, given Δ [N][C]:
 *   r_e = Δ_i                               (+)
 *       = Δ_i / count_i                     (mean; divided once per row)
 *       = (m_e == y_i) ? Δ_i : 0            (max / min; EVERY maximiser receives Δ, NNlib's rule, as gnnmp_propagate_maxmin_grad_f32)
 *   g_e = r_e                               (identity)
 *       = pre_e > 0 ? r_e : 0               (relu; 0 at 0, as gnnmp_act_grad_f32)
 *   dA_i = Σ_{e into i, edge order} g_e
 *   dB_j = Σ_{e out of j, edge order} g_e
 *   dP[i][c]   = dA_i[c]
 *   dP[j][C+c] = dB_j[c] − dA_j[c]
 * m_e and pre_e are RECOMPUTED in both backward passes with exactly the two operations above (the tie test is an equality on floats).  The
 * caller finishes on the dense adjoints: [dW1; dW2] = dP' x (gnnmp_dense_grad_w_f32), db = colsum(dP[:, :C]), dx = dP [W1; W2]
 * (gnnmp_dense_f32, w_layout = 1), dW = [dW1 | dW2].
 *
 *   plan     the graph's plan (rows = destinations); plan_t the plan of the reversed edge index (row j: the edges that leave j, in
 *            original edge order).  Square (n_src == n_dst = N); plan_t of the same height and edge count.  Both are only READ.
 *   job      a HOST record of device pointers:
 *     gnnmp_edge_conv_t       p [N][2C] (read), y [N][C] (every element written), aggr: gnnmp_aggr, act: GNNMP_ACT_IDENTITY | GNNMP_ACT_RELU
 *     gnnmp_edge_conv_grad_t  p [N][2C], y [N][C] the forward's output, dy [N][C] = Δ (all read), dp [N][2C] (every element written; must
 *                             not overlap the inputs), aggr and act as in the forward
 *   C        1 .. 2^20.  Any 4-byte aligned pointers: the kernels use 16- / 8-byte lanes when C % 4 / C % 2 == 0 and every pointer of
 *            the call AND column C inside a row (p + C, dp + C) are aligned alike, 4-byte lanes otherwise.
 * Both exports only launch (the gradient: the destination pass over plan, then the source pass over plan_t, on `stream`): no scratch,
 * no atomics, no host wait; they may be recorded into a HIP graph without an eager call first; N = 0 (an empty graph) launches
 * nothing.  Every row is walked WHOLE, in edge order, by one lane group, whatever its length (the plan's chunks are ignored): the bits
 * are those of the sequential fold for every row — slow for hub rows (in a kNN graph only sources can be hubs).
 * Refused before any HIP call (GNNMP_EINVAL): a NULL plan / plan_t / job / p / y / dy / dp, C outside 1 .. 2^20, an unknown aggr, an act
 * other than identity / relu, a plan with n_src != n_dst, a plan_t whose height or edge count differs from the plan's.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
    const float *p;
    float *y;
    int aggr;
    int act;
} gnnmp_edge_conv_t;
typedef struct {
    const float *p;
    const float *y;
    const float *dy;
    float *dp;
    int aggr;
    int act;
} gnnmp_edge_conv_grad_t;
int gnnmp_edge_conv_f32(const gnnmp_graph_t *plan, const gnnmp_edge_conv_t *job, int64_t C, gnnmp_stream_t stream);
int gnnmp_edge_conv_grad_f32(const gnnmp_graph_t *plan, const gnnmp_graph_t *plan_t, const gnnmp_edge_conv_grad_t *job, int64_t C,
                             gnnmp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * The pullback of CGConv's gated message — cg_conv, GNNlib/src/layers/conv.jl:304-333:
 *   propagate(cg_message, g, +; xi = x, xj = x, e),  cg_message(l, xi, xj, e) = dense_f(z) .* dense_s(z),  z = vcat(xi, xj, e)
 * The forward is gnnmp_propagate_cg_f32 on three PLANAR matrices the caller's dense calls produce from the column blocks of [Wf; Ws]:
 *   fs_i = x [Wf_i; Ws_i]' + [bf; bs]   [N][2C]        fs_j = x [Wf_j; Ws_j]'   [N][2C]        fs_e = e [Wf_e; Ws_e]'   [E][2C], optional
 * columns [0, C) are dense_f's share, columns [C, 2C) dense_s's.  For edge k: j -> i and channel c < C:
 *   f_k = fs_i[i][c]   + fs_j[j][c]   (+ fs_e[k][c])
 *   s_k = fs_i[i][C+c] + fs_j[j][C+c] (+ fs_e[k][C+c])
 *   m_k = sigmoid(f_k) * act(s_k),     y_i = Σ_{k into i} m_k
 *
 * Backward, given Δ [N][C]: f_k and s_k are RECOMPUTED with the same additions in the same order as the forward, and
 *   gf_k = Δ_i * act(s_k) * sigmoid'(f_k)         sigmoid'(f) = sigmoid(f) sigmoid(−f)
 *   gs_k = Δ_i * sigmoid(f_k) * act'(s_k)         act': identity 1 | relu s > 0 (0 at 0, as gnnmp_act_grad_f32) | softplus sigmoid(s) |
 *                                                       tanh (1 − a)(1 + a), a = tanh(s)
 *   dfs_i[i] = Σ_{k into i, edge order}   [gf_k | gs_k]
 *   dfs_j[j] = Σ_{k out of j, edge order} [gf_k | gs_k]
 *   dfs_e[k] = [gf_k | gs_k]                                  (only when wanted)
 * The caller finishes on the dense adjoints, on N and E rows: d[Wf_i; Ws_i] = dfs_i' x and [dbf; dbs] = colsum(dfs_i)
 * (gnnmp_dense_grad_w_f32), d[Wf_j; Ws_j] = dfs_j' x, d[Wf_e; Ws_e] = dfs_e' e, dx = dfs_i [Wf_i; Ws_i] + dfs_j [Wf_j; Ws_j] (+ Δ under
 * the residual), de = dfs_e [Wf_e; Ws_e] (gnnmp_dense_f32, w_layout = 1), dWf = [dWf_i | dWf_j | dWf_e] and dWs likewise.
 *
 *   plan     the graph's plan (rows = destinations); plan_t the plan of the reversed edge index (row j: the edges that leave j, in
 *            original edge order).  Square (n_src == n_dst = N), built WITHOUT plan-added self loops (fs_e has no row for them);
 *            plan_t of the same height and edge count.  Both are only READ.
 *   job      a HOST record of device pointers, gnnmp_cg_conv_grad_t:
 *              fs_i, fs_j [N][2C], fs_e [E][2C] or NULL (no edge features), dy [N][C] = Δ: read
 *              dfs_i, dfs_j [N][2C]: every element written (rows without in-edges / without out-edges: zeros)
 *              dfs_e [E][2C] or NULL (not wanted): every element written, at the edge's ORIGINAL position
 *              act: gnnmp_act, IDENTITY .. TANH — dense_s's activation, as in gnnmp_propagate_cg_f32
 *            Outputs must not overlap the inputs or each other.
 *   C        1 .. 2^19, the forward's bound.  Any 4-byte aligned pointers: the kernels use 16- / 8-byte lanes when C % 4 / C % 2 == 0 and
 *            every pointer of the call AND column C inside a row are aligned alike, 4-byte lanes otherwise.
 * The export only launches — the destination pass over plan, then the source pass over plan_t, on `stream` (csrc/cg_grad.hip): no scratch,
 * no atomics, no host wait, no allocation; it may be recorded into a HIP graph without an eager call first; N = 0 (an empty graph)
 * launches nothing.  Every row is walked WHOLE, in edge order, by one lane group, whatever its length (the plan's chunks are ignored):
 * every sum has the bits of the sequential fold and two calls give equal bits — slow for hub rows.
 * Refused before any HIP call (GNNMP_EINVAL): a NULL plan / plan_t / job / fs_i / fs_j / dy / dfs_i / dfs_j, dfs_e given without fs_e,
 * C outside 1 .. 2^19, an act outside IDENTITY .. TANH, a plan with n_src != n_dst, a plan_t whose height or edge count differs from
 * the plan's, a plan built with self loops (n_total != n_edges).
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
    const float *fs_i, *fs_j, *fs_e;   /* fs_e NULL = no edge features */
    const float *dy;
    float *dfs_i, *dfs_j, *dfs_e;      /* dfs_e NULL = not wanted */
    int act;
} gnnmp_cg_conv_grad_t;
int gnnmp_cg_conv_grad_f32(const gnnmp_graph_t *plan, const gnnmp_graph_t *plan_t, const gnnmp_cg_conv_grad_t *job, int64_t C,
                           gnnmp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * The pullback of NNConv's per-edge-matrix message — nn_conv, GNNlib/src/layers/conv.jl:260-273:
 *   m = propagate(message, g, aggr; xj = x, e),  message(xj, e) = W_k x_j,  W_k = reshape(nn(e)_k, Dout, Din)
 * The forward is gnnmp_propagate_nn_f32 on we = nn(e) [E][Dout * Din], element (o, c) of edge k at we[k][o + Dout * c].  Given the
 * cotangent Δ = dm [N][Dout] of the aggregate, AT THE DESTINATION, for edge k: j -> i at original position k:
 *   dwe[k][o + Dout*c] = dm[i][o] * x[j][c]                                   (the gradient arriving at nn(e): E * Dout * Din values)
 *   dx[j][c]           = Σ_{k out of j} Σ_o we[k][o + Dout*c] * dm[i][o]
 * The export knows no aggregator: `+` passes Δ through; for `mean` the caller pre-scales Δ's rows by 1 / max(indeg, 1) (as the
 * adjoint of gnnmp_propagate_f32 under mean does).  The caller chains dwe through nn's dense adjoints on E rows.
 *
 *   plan_t   the plan of the REVERSED edge index (row j: the edges that leave j, in original edge order; col = the destination,
 *            eid = the original position).  Square, built WITHOUT plan-added self loops (we has no row for them).  Only READ.
 *   job      a HOST record of device pointers, gnnmp_nn_conv_grad_t:
 *              x [N][Din], dm [N][Dout]: read.  we [E][Dout * Din]: read only when dx is wanted; may be NULL when dx is NULL
 *              dx  [N][Din] or NULL (not wanted): every element written (rows without out-edges: zeros)
 *              dwe [E][Dout * Din] or NULL (not wanted): every element written, at the edge's ORIGINAL position
 *            Whichever of dx and dwe is wanted has the same bits whether or not the other is.  Outputs must not overlap the inputs or
 *            each other.
 *   Din, Dout  1 .. 65536, the forward's bounds.  Any 4-byte aligned pointers: the kernel uses 16- / 8-byte lanes when
 *            Dout % 4 / Dout % 2 == 0 and we (when read), dwe (when written) and dm are aligned alike, 4-byte lanes otherwise.
 * One launch over plan_t (csrc/nn_grad.hip): a lane group owns source j, holds x_j, and for every edge that leaves j gathers dm[i],
 * reads W_k once, stores dW_k once and accumulates dx[j] in registers — we is read once, dwe written once, nothing else of E rows
 * moves.  No scratch, no atomics, no host wait, no allocation, nothing owned by the plan written; it may be recorded into a HIP graph
 * without an eager call first.  N = 0 launches nothing; E = 0 with N > 0 writes zeros to dx and touches no row of dwe.  Every row is
 * walked WHOLE by one lane group, whatever its length (the plan's chunks are ignored): two calls give equal bits — slow for hub rows.
 * Summation order of dx[j][c]: products are rounded, then added.  A lane group has G lanes (a power of two, <= 64) of VEC = 4 | 2 | 1
 * floats; lane l owns the outputs o = (t G + l) VEC + q, q < VEC, t = 0, 1, ...  Each lane folds its own products sequentially from
 * 0 — the edges of the row in order, in batches of U (2 for VEC = 4, else 4); within a batch t ascending, then the batch's edges, then
 * q — and the G lane partials are summed by a butterfly (p[l] + p[l ^ m] for m = G/2, G/4, ..., 1).
 * Refused before any HIP call (GNNMP_EINVAL): a NULL plan_t / job / x / dm, dx and dwe both NULL, dx given without we, Din or Dout
 * outside 1 .. 65536, a plan with n_src != n_dst, a plan built with self loops (n_total != n_edges).
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
    const float *x;    /* [N][Din] */
    const float *we;   /* [n_edges][Dout*Din], element (o, c) of edge k at we[k][o + Dout*c]; may be NULL when dx is NULL */
    const float *dm;   /* [N][Dout], the cotangent of the aggregate, at the DESTINATION */
    float *dx;         /* [N][Din] or NULL */
    float *dwe;        /* [n_edges][Dout*Din] or NULL */
} gnnmp_nn_conv_grad_t;
int gnnmp_nn_conv_grad_f32(const gnnmp_graph_t *plan_t, const gnnmp_nn_conv_grad_t *job, int64_t Din, int64_t Dout,
                           gnnmp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * EGNNConv's edge and coordinate steps, forward and pullback — egnn_conv, GNNlib/src/layers/conv.jl:459-495 (csrc/egnn.hip):
 *   x_diff = xi_sub_xj, sqnorm = sum(x_diff .^ 2), x_diff ./ (sqrt(sqnorm) + 1f-6), ϕe(vcat(hi, hj, sqnorm, e)), ϕx scaling the normalised
 *   differences, + for h and mean for x.
 * Edge k: j -> i.  W0 = [A | B | c | D] is ϕe's first weight, split at columns nin, 2 nin, 2 nin + 1.  The caller's dense calls give
 *   P = h A' + b0 [N][hid],  Q = h B' [N][hid],  F = e D' [E][hid] (only with edge features), and
 *   d_k = x_i − x_j    q_k = Σ_a d_k[a]² (a ascending, from 0; products rounded, then added)    r_k = sqrt(q_k)    n_k = d_k / (r_k + 1e-6)
 *
 *   gnnmp_egnn_edge_f32   K1, in ORIGINAL edge order from s, t: q [E], z0_k = ((P_i + Q_j) + q_k c) (+ F_k), a0 = act(z0) [E][hid]; z0 is
 *                         stored only when the pointer is non-NULL (a gradient is wanted).  act: any gnnmp_act, evaluated by the device
 *                         function of gnnmp_bias_act_f32: a0 has the bits of gnnmp_bias_act_f32(z0, NULL, act).  Indices are not validated.
 *   gnnmp_egnn_coord_f32  K2, one pass over the plan: x'_i = x_i + (1 / deg_i) Σ_{k into i} mx_k n_k, deg_i = the in-degree; a row without
 *                         in-edges gets x'_i = x_i.  n_k is recomputed from x; nothing of E rows but mx [E] is read, only x' written.
 *   gnnmp_egnn_coord_grad_f32   K3, given Δx' = dxo [N][Dx]:
 *                           dmx_k = (Σ_a n_k[a] Δx'_i[a]) / deg_i                                            (dmx non-NULL)
 *                           g_k = (mx_k / deg_i) Δx'_i,  den = r_k + 1e-6
 *                           dd_k = (g_k / den − d_k ((d_k · g_k) / (r_k den²))) + (2 dq_k) d_k
 *                           dx_i = (Δx'_i + Σ_{k into i} dd_k) − Σ_{k out of i} dd_k                           (dx non-NULL)
 *                         where dq [E] is the cotangent that reaches q through z0 (dz0 c).  WHERE q_k == 0 (a self loop, coincident points)
 *                         THE n-PATH TERMS ARE DEFINED AS 0: dd_k = 2 dq_k d_k = 0 and dmx_k = 0.  The reference's AD gives Inf * 0 = NaN
 *                         there (the derivative of sqrt at 0); this is a convention, not a derivative.  One launch: the lane group of node i
 *                         walks row i of plan (the edges into i) and, for dx, row i of plan_t (the edges out of i; it gathers x, Δx', the
 *                         in-degree of the destination from plan, mx[eid] and dq[eid]).  Either output has the same bits whether or not
 *                         the other is asked for.
 *   gnnmp_act_grad_z_f32  dz = dy ⊙ act'(z) from the PRE-activation z, n elements, any gnnmp_act: identity 1 | relu z > 0 (0 at 0) |
 *                         softplus sigmoid(z) | tanh (1 − a)(1 + a), a = tanh(z) | swish σ(z) (1 + z (1 − σ(z))).  (gnnmp_act_grad_f32
 *                         works from the OUTPUT y and covers identity and relu only.)
 *
 * Device pointers travel in const HOST records.  All four only launch on `stream`: no atomics, no scratch, no host wait, no allocation,
 * nothing owned by a plan written; each may be recorded into a HIP graph without an eager call first; two calls give equal bits.  Outputs must
 * not overlap the inputs or each other.  Any 4-byte aligned pointers: K1 uses 16- / 8-byte lanes when hid % 4 / hid % 2 == 0 and P, Q, F,
 * c, a0 and z0 are aligned alike (a second feature tile beyond 256 features), gnnmp_act_grad_z_f32 16-byte lanes when dy, z and dz are
 * 16-byte aligned; K2 and K3 keep a node's Dx <= 16 coordinates in registers and use 4-byte accesses.
 * K2 / K3 rows are walked WHOLE by one lane group, whatever their length (the plan's chunks are ignored) — slow for hub rows.  Summation
 * order of a row: the group has G lanes, G = the smallest power of two >= the plan's mean row length (at most 64); lane l folds the
 * row's slots l, l + G, l + 2G, ... sequentially from 0, slots in plan order (= original edge order), and the G lane partials are summed
 * by a butterfly (p[l] + p[l ^ m] for m = G/2, G/4, ..., 1).
 * N = 0 launches nothing; E = 0 with N > 0 writes x' = x and dx = Δx' and touches no edge array.
 * Refused before any HIP call (GNNMP_EINVAL): a NULL job or required pointer (K1: s, t, x, P, Q, c, q, a0; K2: plan, x, mx, xo; K3: plan, x,
 * dxo, dmx and dx both NULL, dx without plan_t / mx / dq; mx and dq may be NULL on a plan without edges; act_grad_z: dy, dz, z unless act is IDENTITY), idx_bytes not 4 | 8, hid
 * outside 1 .. 2^19, Dx outside 1 .. 16, an act outside IDENTITY .. SWISH, negative E or n, a plan with n_src != n_dst, a plan_t whose
 * height or edge count differs from the plan's, a plan built with self loops of its own (n_total != n_edges: mx has no entry for them).
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
    const void *s, *t;         /* [E] the edge index as the graph holds it: edge k goes s[k] -> t[k] */
    int idx_bytes, index_base; /* 8 | 4, 1 | 0 */
    const float *x;            /* [N][Dx] */
    const float *P, *Q;        /* [N][hid] */
    const float *F;            /* [E][hid] or NULL (no edge features) */
    const float *c;            /* [hid] */
    float *q;                  /* [E] */
    float *a0;                 /* [E][hid] */
    float *z0;                 /* [E][hid] or NULL (not wanted) */
    int act;
} gnnmp_egnn_edge_t;
int gnnmp_egnn_edge_f32(const gnnmp_egnn_edge_t *job, int64_t E, int64_t hid, int64_t Dx, gnnmp_stream_t stream);

typedef struct {
    const float *x;    /* [N][Dx] */
    const float *mx;   /* [E] */
    float *xo;         /* [N][Dx] = x' */
} gnnmp_egnn_coord_t;
int gnnmp_egnn_coord_f32(const gnnmp_graph_t *plan, const gnnmp_egnn_coord_t *job, int64_t Dx, gnnmp_stream_t stream);

typedef struct {
    const float *x;    /* [N][Dx] */
    const float *dxo;  /* [N][Dx] = Δx' */
    const float *mx;   /* [E]; may be NULL when dx is NULL */
    const float *dq;   /* [E]; may be NULL when dx is NULL */
    float *dmx;        /* [E] or NULL (not wanted) */
    float *dx;         /* [N][Dx] or NULL (not wanted) */
} gnnmp_egnn_coord_grad_t;
int gnnmp_egnn_coord_grad_f32(const gnnmp_graph_t *plan, const gnnmp_graph_t *plan_t, const gnnmp_egnn_coord_grad_t *job, int64_t Dx,
                              gnnmp_stream_t stream);

typedef struct {
    const float *dy;   /* [n] */
    const float *z;    /* [n] the pre-activation; may be NULL for IDENTITY */
    float *dz;         /* [n] */
    int act;
} gnnmp_act_grad_z_t;
int gnnmp_act_grad_z_f32(const gnnmp_act_grad_z_t *job, int64_t n, gnnmp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * GMMConv (MoNet) on fused mixture-weight kernels, forward and pullback — gmm_conv, GNNlib/src/layers/conv.jl:372-401 (csrc/gmm.hip):
 *   w = exp(sum over d of ((e − mu)² / 2) .* sigma_inv²)  (1, K, E),  propagate(e_mul_xj, g, mean; xj = dense_x(x) as (out, K, N), e = w),
 *   mean over the K kernels, σ.(m .+ bias), optional residual.
 * Edge e: j -> i, kernel k < K, channel c < C.  The caller provides w [E][K] (gnnmp_gmm_weights_f32 with C = 1: one number per edge and
 * kernel) and xk = x dense_x_weight' [N][K C], kernel k's block at k C (gnnmp_dense_f32).  Neither [E][K C] nor [N][K C] is written.
 *
 *   gnnmp_gmm_conv_f32         acc_ikc = Σ_{e into i, edge order, from 0} w[e][k] * xk[j][k C + c]     A MULTIPLY AND AN ADD per edge: the
 *                                                                                                     product is rounded, then added
 *                              m_ikc = acc_ikc / deg_i (deg_i = the in-degree; a row without in-edges keeps 0)
 *                              z_ic = (((m_i0c + m_i1c) + ...) + m_i,K−1,c) / K (+ bias_c)            y = act(z), any gnnmp_act, by the device
 *                              function of gnnmp_bias_act_f32.  z is stored only when the pointer is non-NULL (a gradient is wanted).
 *                              One lane group finishes one destination row: its lanes run over the channels, each holds K accumulators per
 *                              channel in registers; the K weights of an edge are read once per edge, at the edge's original position.
 *   gnnmp_gmm_conv_grad_f32    given dz [N][C] = Δ ⊙ act'(z) (gnnmp_act_grad_z_f32), with q_i = 1 / (K max(deg_i, 1)), t_ic = q_i * dz_ic:
 *                              dxk[j][k C + c] = Σ_{e out of j, edge order, from 0} w[e][k] * t_ic    (products rounded, then added)
 *                              dw[e][k]        = Σ_c xk[j][k C + c] * t_ic
 *                              One walk of plan_t: the lane group of source j keeps xk[j] in registers and reads, per out-edge, dz_i, w_e
 *                              and deg_i — the degree from `plan`; plan_t only orders the walk.  dxk[j] is accumulated in registers and
 *                              written once (a row without out-edges: zeros); dw is written at the edge's original position.  Order of
 *                              dw's sum: a lane group has G lanes (a power of two <= 64) of VEC = 4 | 2 | 1 channels; lane l owns channels
 *                              (T G + l) VEC + q, q < VEC, of tile T.  Within a tile the lane adds its products from 0 in ascending q, the
 *                              G lane sums go through a butterfly (p[l] + p[l ^ m], m = G/2, ..., 1); tiles (more than one only when
 *                              C > 64 VEC) are added in ascending T.  G and VEC follow from C and the pointers' alignment only.  Whichever
 *                              of dxk and dw is wanted has the same bits whether or not the other is.
 *   gnnmp_gmm_weights_grad_f32 the pullback of gnnmp_gmm_weights_f32 (C = 1): with g_ek = dw[e][k] * w[e][k] and δ = e[e][d] − mu[k][d],
 *                              de[e][d]    =  Σ_k (g_ek δ) * sinv[k][d]²          k ascending from 0; one thread an edge
 *                              dmu[k][d]   = −Σ_e (g_ek δ) * sinv[k][d]²
 *                              dsinv[k][d] =  Σ_e (g_ek δ²) * sinv[k][d]
 *                              dmu / dsinv are a two-stage fold without atomics.  THE SLICE RULE: block b < GNNMP_GMM_PARTS folds the edges
 *                              [b L, min(E, (b + 1) L)), L = ceil(E / GNNMP_GMM_PARTS), into part[b][0][k][d] (dmu) and part[b][1][k][d]
 *                              (dsinv): lane l of a wave folds the slice's edges l, l + 64, ... sequentially from 0, the 64 lane sums go
 *                              through a butterfly; then ONE block adds part[0], part[1], ... in index order from 0.  No value passes
 *                              through more than ceil(L / 64) + 6 + GNNMP_GMM_PARTS additions — at most L + GNNMP_GMM_PARTS, the depth to
 *                              put into a summation bound.  Every element of part is written (an empty slice: zeros).
 *
 *   plan     the graph's plan (rows = destinations); plan_t the plan of the reversed edge index (row j: the edges that leave j, in
 *            original edge order).  Square (n_src == n_dst = N), built WITHOUT plan-added self loops (w has no row for them); plan_t of
 *            the same height and edge count.  Both are only READ; the plans' chunks are ignored.
 *   job      a const HOST record of device pointers:
 *              gnnmp_gmm_conv_t          w [E][K], xk [N][K C]: read; bias [C] or NULL; y [N][C]: every element written; z [N][C] or NULL
 *                                        (not wanted): every element written; act: gnnmp_act, IDENTITY .. SWISH
 *              gnnmp_gmm_conv_grad_t     dz [N][C]: read; w [E][K]: read only when dxk is wanted; xk [N][K C]: read only when dw is wanted;
 *                                        dxk [N][K C] or NULL, dw [E][K] or NULL: every element written
 *              gnnmp_gmm_weights_grad_t  e [E][ein], mu, sinv [K][ein], w, dw [E][K]: read; de [E][ein] or NULL; dmu, dsinv [K][ein], both
 *                                        or neither; part [GNNMP_GMM_PARTS][2][K][ein] floats, caller-owned, needed with dmu
 *            Outputs must not overlap the inputs or each other.
 *   K        1 .. 16.   C  1 .. 2^19 with K C <= 2^20.   ein  1 .. 64.   Any 4-byte aligned pointers: the row kernels use 16- / 8-byte
 *            lanes when C % 4 / C % 2 == 0 and xk, bias, y, z (forward) or xk, dz, dxk (pullback) are aligned alike, 4-byte lanes otherwise.
 * All three only launch on `stream`: no atomics, no allocation, no host wait, nothing owned by a plan written; each may be recorded into
 * a HIP graph without an eager call first; two calls give equal bits.  N = 0 (the row exports) or E = 0 (gnnmp_gmm_weights_grad_f32)
 * launches nothing and returns GNNMP_OK — the caller zero-fills dmu / dsinv of a graph without edges; E = 0 with N > 0 gives
 * y = act(bias) and dxk = 0.  Every row is walked WHOLE by one lane group, whatever its length: slow for hub rows.
 * Refused before any HIP call (GNNMP_EINVAL): a NULL plan / plan_t / job; forward: a NULL xk / y, a NULL w on a plan with edges; pullback:
 * dxk and dw both NULL, a NULL dz, dxk without w (on a plan with edges), dw without xk; weights: de, dmu and dsinv all NULL, only one of
 * dmu / dsinv, dmu without part, negative E, and with E > 0 a NULL e / mu / sinv / w / dw; K outside 1 .. 16, C outside 1 .. 2^19 or
 * K C > 2^20, ein outside 1 .. 64, an act outside IDENTITY .. SWISH, a plan with n_src != n_dst, a plan_t whose height or edge count
 * differs from the plan's, a plan built with self loops of its own (n_total != n_edges).
 * ---------------------------------------------------------------------------------------------- */
#define GNNMP_GMM_PARTS 256 /* partial blocks of gnnmp_gmm_weights_grad_f32's dmu / dsinv fold */
typedef struct {
    const float *w;    /* [E][K] */
    const float *xk;   /* [N][K*C] */
    const float *bias; /* [C] or NULL */
    float *y;          /* [N][C] */
    float *z;          /* [N][C] or NULL (not wanted) */
    int act;
} gnnmp_gmm_conv_t;
int gnnmp_gmm_conv_f32(const gnnmp_graph_t *plan, const gnnmp_gmm_conv_t *job, int64_t K, int64_t C, gnnmp_stream_t stream);

typedef struct {
    const float *w;    /* [E][K]; may be NULL when dxk is NULL */
    const float *xk;   /* [N][K*C]; may be NULL when dw is NULL */
    const float *dz;   /* [N][C] */
    float *dxk;        /* [N][K*C] or NULL (not wanted) */
    float *dw;         /* [E][K] or NULL (not wanted) */
} gnnmp_gmm_conv_grad_t;
int gnnmp_gmm_conv_grad_f32(const gnnmp_graph_t *plan, const gnnmp_graph_t *plan_t, const gnnmp_gmm_conv_grad_t *job, int64_t K, int64_t C,
                            gnnmp_stream_t stream);

typedef struct {
    const float *e;    /* [E][ein] */
    const float *mu;   /* [K][ein] */
    const float *sinv; /* [K][ein] */
    const float *w;    /* [E][K] */
    const float *dw;   /* [E][K] */
    float *de;         /* [E][ein] or NULL (not wanted) */
    float *dmu;        /* [K][ein] or NULL (not wanted; then dsinv is NULL too) */
    float *dsinv;      /* [K][ein] or NULL */
    float *part;       /* [GNNMP_GMM_PARTS][2][K][ein], needed with dmu / dsinv */
} gnnmp_gmm_weights_grad_t;
int gnnmp_gmm_weights_grad_f32(const gnnmp_gmm_weights_grad_t *job, int64_t E, int64_t ein, int64_t K, gnnmp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * MEGNetConv on fused edge-update kernels, forward and pullback — megnet_conv, GNNlib/src/layers/conv.jl:356-368 (csrc/megnet.hip):
 *   ē = ϕe(vcat(xi, xj, e)),  xᵉ = aggregate_neighbors(g, aggr, ē) (msgpass.jl:145-149),  x̄ = ϕv(vcat(x, xᵉ))  ->  (x̄, ē).
 * Edge k: j -> i, feature c < hid.  ϕe's first weight W0 = [A | B | D] is split at columns in and 2 in; the caller provides
 * P = x A' + b0, Q = x B' [N][hid] and F = e D' [E][hid] (gnnmp_dense_f32).  No [E][in] gather of x and no [E][2 in + ein] row exists.
 *
 *   gnnmp_megnet_edge_f32       z0_k = (P_i + Q_j) + F_k  (P_i + Q_j alone without F),  a0_k = act(z0_k) by the device function of
 *                               gnnmp_bias_act_f32: a0 has the bits of gnnmp_bias_act_f32(z0, NULL, act).  One pass over the plan: the
 *                               lane group of destination i keeps P_i in registers; both outputs are stored at the edge's original
 *                               position.  z0 is stored only when the pointer is non-NULL (a gradient is wanted).
 *   gnnmp_megnet_edge_grad_f32  dz0_k = da0_k ⊙ act'(z_k), the formulas of gnnmp_act_grad_z_f32 (its device function); IDENTITY: dz0 = da0
 *                               and z is not read (it may be NULL).  For RELU a0 MAY BE PASSED AS z: the mask z > 0 is the mask a0 > 0.
 *                               Pass 1, over plan:   dz0 stored at the edge's original position when wanted, and
 *                                                    dP_i = Σ_{k into i, plan order, from 0} dz0_k
 *                               Pass 2, over plan_t: dQ_j = Σ_{k out of j, plan order, from 0} dz0_k, dz0_k recomputed from da0 and z.
 *                               Each of dz0, dP, dQ has the same bits whether or not the others are asked for; a row without in-edges
 *                               (out-edges) gets dP_i = 0 (dQ_j = 0).
 *   gnnmp_aggregate_grad_f32    NNlib's pullback of scatter(aggr, m, t), y = aggregate_neighbors(g, aggr, m), Δ = dy: the term of edge k
 *                                   + :          Δ_i
 *                                   mean :       Δ_i / deg_i, divided ONCE per row (deg_i = the row's length), then copied
 *                                   max / min :  Δ_i where m_k == y_i, 0 elsewhere — EVERY tying copy gets the whole Δ (the reference's rule)
 *                               dm_k = acc_k + term when acc is given (the cotangent that reaches m directly: summed here, not by a
 *                               separate add), the term alone otherwise.  One pass over the plan with Δ_i (and y_i) in registers, dm stored
 *                               at the edge's original position.
 *
 *   plan     the graph's plan (rows = destinations); plan_t the plan of the reversed edge index (row j: the edges that leave j).  The two
 *            MEGNet exports want them square (n_src == n_dst = N) and of the same height and edge count; gnnmp_aggregate_grad_f32 walks
 *            the n_dst rows of any plan.  All want a plan built WITHOUT plan-added self loops (the E-row arrays have no row for them).
 *            Plans are only READ; their chunks are ignored.
 *   job      a const HOST record of device pointers:
 *              gnnmp_megnet_edge_t       P, Q [N][hid]: read; F [E][hid] or NULL; a0 [E][hid]: every element written; z0 [E][hid] or NULL
 *                                        (not wanted): every element written; act: gnnmp_act, IDENTITY .. SWISH
 *              gnnmp_megnet_edge_grad_t  da0, z [E][hid]: read (z: NULL allowed for IDENTITY); dz0 [E][hid] or NULL; dP, dQ [N][hid], both
 *                                        or neither (then plan_t may be NULL): every element written; at least one output; act as above
 *              gnnmp_aggregate_grad_t    dy [n_dst][D]: read; m [E][D], y [n_dst][D]: read for max / min only (NULL allowed otherwise);
 *                                        acc [E][D] or NULL; dm [E][D]: every element written
 *            Outputs must not overlap the inputs or each other.
 *   hid, D   1 .. 2^19.  Any 4-byte aligned pointers: 16- / 8-byte lanes when hid % 4 / hid % 2 == 0 and every pointer of the call is
 *            aligned alike, 4-byte lanes otherwise; lanes run over the features (a second feature tile beyond 64 lanes), a row's slots
 *            are folded sequentially in plan order.
 * All three only launch on `stream`: no atomics, no allocation, no host wait, nothing owned by a plan written; each may be recorded into
 * a HIP graph without an eager call first; two calls give equal bits.  N = 0 launches nothing and returns GNNMP_OK; E = 0 with N > 0
 * writes zeros to dP / dQ and touches no E-row array (their pointers may then be NULL).  Every row is walked WHOLE by one lane group,
 * whatever its length: slow for hub rows.
 * Refused before any HIP call (GNNMP_EINVAL): a NULL plan / job; a NULL P / Q; on a plan with edges a NULL a0, da0, z (act not IDENTITY),
 * dy, dm, and m / y under max / min; dz0, dP and dQ all NULL, only one of dP / dQ, dQ without plan_t; hid / D outside 1 .. 2^19; an act
 * outside IDENTITY .. SWISH, an aggr outside GNNMP_SUM .. GNNMP_MIN; a plan with n_src != n_dst (the two MEGNet exports), a plan_t whose
 * height or edge count differs from the plan's, a plan built with self loops of its own (n_total != n_edges).
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
    const float *P;    /* [N][hid] */
    const float *Q;    /* [N][hid] */
    const float *F;    /* [E][hid] or NULL */
    float *a0;         /* [E][hid] */
    float *z0;         /* [E][hid] or NULL (not wanted) */
    int act;
} gnnmp_megnet_edge_t;
int gnnmp_megnet_edge_f32(const gnnmp_graph_t *plan, const gnnmp_megnet_edge_t *job, int64_t hid, gnnmp_stream_t stream);

typedef struct {
    const float *da0;  /* [E][hid] */
    const float *z;    /* [E][hid]; NULL allowed for IDENTITY; a0 allowed for RELU */
    float *dz0;        /* [E][hid] or NULL (not wanted) */
    float *dP;         /* [N][hid] or NULL (not wanted; then dQ is NULL too) */
    float *dQ;         /* [N][hid] or NULL */
    int act;
} gnnmp_megnet_edge_grad_t;
int gnnmp_megnet_edge_grad_f32(const gnnmp_graph_t *plan, const gnnmp_graph_t *plan_t, const gnnmp_megnet_edge_grad_t *job, int64_t hid,
                               gnnmp_stream_t stream);

typedef struct {
    const float *dy;   /* [n_dst][D] */
    const float *m;    /* [E][D]; max / min only */
    const float *y;    /* [n_dst][D]; max / min only */
    const float *acc;  /* [E][D] or NULL */
    float *dm;         /* [E][D] */
} gnnmp_aggregate_grad_t;
int gnnmp_aggregate_grad_f32(const gnnmp_graph_t *plan, const gnnmp_aggregate_grad_t *job, int aggr, int64_t D, gnnmp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Attention readouts on fused segment kernels, forward and pullback — GlobalAttentionPool, GNNlib/src/layers/pool.jl:7-12, and Set2Set,
 * pool.jl:29-43 (csrc/readout.hip).  Both are a per-graph softmax-weighted sum over the graph's CONTIGUOUS rows [seg_ptr[g], seg_ptr[g+1])
 * (what gnnmp_segment_bounds writes): no [N] array of logits or weights and no [N][D] product is written.  Graph g, row n, feature d.
 *
 *   gnnmp_segment_attn_pool_f32   the logits s_n:
 *                                   QUERY (Dg = 0, q given; pool.jl:37-39)  s_n = Σ_d q_g[d] x_n[d]: each lane sums its own features in
 *                                                                           ascending d from 0, the lanes' partials are folded by an xor
 *                                                                           butterfly (a fixed order that depends on D and the alignment)
 *                                   GATE (gate given; pool.jl:8-10)         s_n = gate_n (Dg = 1, one weight for every feature) or
 *                                                                           s_n[d] = gate_n[d] (Dg = D, a softmax per channel)
 *                                 then THREE sweeps over the segment, each in node order (not an online rescaling):
 *                                   m_g   = max_n s_n                       (from -Inf)
 *                                   den_g = Σ_n expf(s_n - m_g)             (from 0)
 *                                   r_g   = Σ_n α_n x_n                     (from 0),  α_n = expf(s_n - m_g) / den_g
 *                                 stats[g][j] = (m_g, den_g), j < max(Dg, 1): one pair per graph, or per channel for Dg = D.  An EMPTY
 *                                 segment gives r_g = 0 (NNlib.scatter's zero) and stats (0, 0).
 *   gnnmp_segment_attn_pool_grad_f32   ONE sweep in node order, α_n recomputed from stats by the expression above (the same bits):
 *                                   c_g = Σ_d dr_g[d] r_g[d],  t_n = Σ_d dr_g[d] x_n[d]    (summed like the QUERY logit)
 *                                   QUERY   ds_n = α_n (t_n - c_g),  dq_g = Σ_n ds_n x_n (node order, from 0),
 *                                           dx_n = (base_n + α_n dr_g) + ds_n q_g
 *                                   Dg = 1  dgate_n = α_n (t_n - c_g),  dx_n = base_n + α_n dr_g
 *                                   Dg = D  dgate_n[d] = (α_n[d] dr_g[d]) (x_n[d] - r_g[d]),  dx_n[d] = base_n[d] + α_n[d] dr_g[d]
 *                                 without base its addition is left out.  base MAY BE dx ITSELF (each element is read, then written, by one
 *                                 lane): T Set2Set iterations accumulate into one dx with no separate add.  dq, dx, dgate are each optional:
 *                                 a NULL output is not computed and the others keep their bits.  An empty segment gives dq_g = 0.
 *   gnnmp_lstm_pointwise_grad_f32      pullback of gnnmp_lstm_pointwise_f32: a = gx + gh + b recomputed by its expressions,
 *                                   i, f, o = σ(a_i, a_f, a_o), g̃ = tanhf(a_c), T = tanhf(f c + i g̃);   dc'_tot = dc' + dh' o (1 - T²)
 *                                   (dc' = 0 when dcn is NULL: the last step)
 *                                   da_i = dc'_tot g̃ (i (1 - i)),  da_f = dc'_tot c (f (1 - f)),  da_c = dc'_tot i (1 - g̃²),
 *                                   da_o = dh' T (o (1 - o)),  dc = dc'_tot f.     da [N][4D] (gate order i, f, c, o) is the cotangent of gx
 *                                   AND of gh; colsum(da) that of b.
 *
 *   job      a const HOST record of device pointers:
 *              gnnmp_segment_attn_t       x [N][D], seg_ptr int64 [G+1] (0-based row offsets, ascending; clamped into [0, N] by the kernel):
 *                                         read; EXACTLY ONE of q [G][D] and gate [N][Dg]; r [G][D], stats [G][max(Dg,1)][2]: every element
 *                                         written
 *              gnnmp_segment_attn_grad_t  dr [G][D], x, seg_ptr, q or gate, r, stats (the forward's): read; base [N][D] or NULL (needs dx);
 *                                         dq [G][D] (QUERY only), dx [N][D], dgate [N][Dg] (GATE only), each or NULL, at least one of the
 *                                         mode's two: every element written
 *              gnnmp_lstm_grad_t          gx, gh [N][4D], b [4D] or NULL, c [N][D] (the cell state that ENTERED the step), dh [N][D]: read;
 *                                         dcn [N][D] or NULL; da [N][4D], dc [N][D]: every element written
 *            Outputs must not overlap the inputs or each other, base == dx excepted.
 *   D        1 .. GNNMP_READOUT_MAX_D (the LSTM pullback: 1 .. 2^20).  Any 4-byte aligned pointers: 16- / 8-byte lanes when D % 4 / D % 2
 *            == 0 and every [·][D] pointer of the call is aligned alike, 4-byte lanes otherwise.  ONE lane group (the smallest power of
 *            two that holds the row's lanes, at most 64) finishes a graph, 4 rows in flight.  A row wider than 64 lanes is covered in
 *            feature tiles by the SAME group, and the logit loop then reads the whole row once per tile (quadratic in the tile count).
 * All three only launch on `stream`: no atomics, no allocation, no host wait, no scratch; each may be recorded into a HIP graph without
 * an eager call first; two calls give equal bits.  G = 0 or N = 0 launches nothing, writes nothing and returns GNNMP_OK.  A SEGMENT OF ANY
 * LENGTH IS WALKED BY ITS ONE LANE GROUP: a whole-graph readout of millions of rows is slow.
 * Refused before any HIP call (GNNMP_EINVAL), each message naming its export: a NULL job; a NULL x (N > 0), seg_ptr, r, stats, dr, gx, gh,
 * c, dh, da, dc; both or neither of q and gate; Dg outside {0, 1, D}, Dg = 0 with gate or Dg > 0 with q; D outside its range; a negative
 * N or G; in the pullback no output, dgate in QUERY mode, dq in GATE mode, base without dx.
 * ---------------------------------------------------------------------------------------------- */
#define GNNMP_READOUT_MAX_D 4096
typedef struct {
    const float *x;          /* [N][D] */
    const int64_t *seg_ptr;  /* [G+1] */
    const float *q;          /* [G][D], QUERY mode (Dg = 0); else NULL */
    const float *gate;       /* [N][Dg], GATE mode (Dg = 1 | D); else NULL */
    float *r;                /* [G][D] */
    float *stats;            /* [G][max(Dg,1)][2]: (max, denominator) */
} gnnmp_segment_attn_t;
int gnnmp_segment_attn_pool_f32(const gnnmp_segment_attn_t *job, int64_t N, int64_t G, int64_t D, int64_t Dg, gnnmp_stream_t stream);

typedef struct {
    const float *dr;         /* [G][D] */
    const float *x;          /* [N][D] */
    const int64_t *seg_ptr;  /* [G+1] */
    const float *q;          /* [G][D] or NULL */
    const float *gate;       /* [N][Dg] or NULL */
    const float *r;          /* [G][D], the forward's */
    const float *stats;      /* [G][max(Dg,1)][2], the forward's */
    const float *base;       /* [N][D] or NULL; may be dx */
    float *dq;               /* [G][D] or NULL; QUERY mode */
    float *dx;               /* [N][D] or NULL */
    float *dgate;            /* [N][Dg] or NULL; GATE mode */
} gnnmp_segment_attn_grad_t;
int gnnmp_segment_attn_pool_grad_f32(const gnnmp_segment_attn_grad_t *job, int64_t N, int64_t G, int64_t D, int64_t Dg,
                                     gnnmp_stream_t stream);

typedef struct {
    const float *gx;         /* [N][4D] */
    const float *gh;         /* [N][4D] */
    const float *b;          /* [4D] or NULL */
    const float *c;          /* [N][D]: the cell state that entered the step */
    const float *dh;         /* [N][D]: cotangent of h' */
    const float *dcn;        /* [N][D] or NULL: cotangent of c' from the next step */
    float *da;               /* [N][4D] */
    float *dc;               /* [N][D] */
} gnnmp_lstm_grad_t;
int gnnmp_lstm_pointwise_grad_f32(const gnnmp_lstm_grad_t *job, int64_t N, int64_t D, gnnmp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * The polynomial layers and the GRU cell, forward and pullback (csrc/poly_conv.hip) — what cheb_conv, GNNlib/src/layers/conv.jl:83-98,
 * d_conv, conv.jl:696-724, and gated_graph_conv, conv.jl:218-233, need beyond the existing exports to train.
 *
 *   gnnmp_poly_hop_f32   one step of a three-term recurrence over a plan, in one launch.  Row i of the plan, its slots k in plan order:
 *                            agg_i = Σ_k w_slot[k] * (z[col[k]] * ss_slot[k])          from 0, slot by slot; a NULL factor is left out
 *                            agg_i = agg_i * scale_dst[i]                              when scale_dst is given
 *                            out_i = alpha * agg_i
 *                            out_i = out_i + beta * self_i                             when self is given
 *                            out_i = out_i + gamma * prev_i                            when prev is given
 *                            out_i = out_i + add_i                                     when add is given
 *                        IN THIS ORDER, every product and every sum rounded on its own: the library is built with -ffp-contract=off and
 *                        the kernel has no fmaf, so no two of these steps are contracted.  w_slot and ss_slot mean what they mean in
 *                        gnnmp_propagate_slots_f32 (gnnmp_plan_slot_gather_f32 makes them) and the per-slot factor and the fold are
 *                        that export's expressions: with alpha = 1 and no self, prev or add, out has ITS BITS on every row the plan does
 *                        not split (1 * agg is agg).  A row without slots gets the epilogue of agg = 0.
 *                        cheb_conv's order k >= 3 is alpha = -4/λ, beta = 2 (2/λ - 1), gamma = -1 with self = Z_{k-1}, prev = Z_{k-2};
 *                        d_conv's `2 * step - T0` is alpha = 2, gamma = -1, prev = T0; over the transposed plan, with add = G_k, the same
 *                        call is a step of the pullback (Clenshaw: B_k = G_k + 2 L̃ᵀ B_{k+1} - B_{k+2}).
 *   gnnmp_gru_pointwise_grad_f32   pullback of gnnmp_gru_pointwise_f32: with a_r = gx_r + gh_r + b_r, a_z = gx_z + gh_z + b_z,
 *                        r = σ(a_r), z = σ(a_z), h~ = tanhf(gx_n + r * gh_n + b_n) recomputed by its expressions (its additions, in its
 *                        order) and Δ = dout:
 *                            dh     = base + Δ z                         (Δ z alone without base)
 *                            dz_pre = (Δ (h - h~)) (z (1 - z))
 *                            dn_pre = (Δ (1 - z)) (1 - h~ h~)
 *                            dr_pre = (dn_pre gh_n) (r (1 - r))
 *                            dgx = (dr_pre, dz_pre, dn_pre),   dgh = (dr_pre, dz_pre, dn_pre r)        gate order r, z, candidate
 *                        dgx is the cotangent of gx = Wi m, dgh that of gh = Wh h; colsum(dgx) is that of b.  dh is only the DIRECT
 *                        term of h: the caller adds dgh Wh.
 *
 *   plan     any plan (rows = n_dst destinations, z has n_src rows); only READ, its chunks are ignored; no eid is read, so a plan built
 *            with self loops of its own is taken (their w_slot entry is 1, as gnnmp_plan_slot_gather_f32 writes it).
 *   job      a const HOST record of device pointers and scalars:
 *              gnnmp_poly_hop_t   z [n_src][D]: read; w_slot, ss_slot [n_total] (plan slot order), scale_dst [n_dst], self, prev, add
 *                                 [n_dst][D]: read, each may be NULL; alpha, beta, gamma; out [n_dst][D]: every element written.
 *                                 out MAY BE prev OR add (each element is read by the lane that then writes it); out may NOT be z or
 *                                 self (z is gathered by other lanes; cheb_conv passes one array as both).  A term is applied when its
 *                                 pointer is given, whatever its coefficient.
 *              gnnmp_gru_grad_t   gx, gh [N][3D], b [3D] or NULL, h [N][D] (the state that ENTERED the cell), dout [N][D]: read; base
 *                                 [N][D] or NULL, MAY BE dh; dgx, dgh [N][3D], dh [N][D]: every element written
 *            Outputs must not overlap the inputs or each other beyond what is said above.
 *   D        the hop: 1 .. 2^19; any 4-byte aligned pointers: 16- / 8-byte lanes when D % 4 / D % 2 == 0 and z, self, prev, add and out are
 *            aligned alike, 4-byte lanes otherwise; lanes run over the features (a second feature tile beyond 64 lanes), a row's slots
 *            are folded sequentially in plan order.  The GRU pullback: 1 .. 2^20, one thread an element.
 * Both only launch on `stream`: no atomics, no allocation, no host wait, no scratch, nothing owned by a plan written; each may be
 * recorded into a HIP graph without an eager call first; two calls give equal bits.  n_dst = 0 / N = 0 launches nothing and returns
 * GNNMP_OK.  EVERY ROW IS WALKED WHOLE BY ONE LANE GROUP, whatever its length: correct, and slow for hub rows (where
 * gnnmp_propagate_slots_f32 splits them).
 * Refused before any HIP call (GNNMP_EINVAL), each message naming its export: a NULL plan or job; a NULL z or out; D outside its range;
 * out == z or out == self; beta != 0 with a NULL self, gamma != 0 with a NULL prev; a NULL gx, gh, h, dout, dgx, dgh or dh; a negative N.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
    const float *z;          /* [n_src][D] */
    const float *w_slot;     /* [n_total], plan slot order, or NULL */
    const float *ss_slot;    /* [n_total], plan slot order, or NULL */
    const float *scale_dst;  /* [n_dst] or NULL */
    const float *self;       /* [n_dst][D] or NULL */
    const float *prev;       /* [n_dst][D] or NULL; may be out */
    const float *add;        /* [n_dst][D] or NULL; may be out */
    float alpha, beta, gamma;
    float *out;              /* [n_dst][D] */
} gnnmp_poly_hop_t;
int gnnmp_poly_hop_f32(const gnnmp_graph_t *plan, const gnnmp_poly_hop_t *job, int64_t D, gnnmp_stream_t stream);

typedef struct {
    const float *gx;         /* [N][3D] */
    const float *gh;         /* [N][3D] */
    const float *b;          /* [3D] or NULL */
    const float *h;          /* [N][D]: the state that entered the cell */
    const float *dout;       /* [N][D]: cotangent of h' */
    const float *base;       /* [N][D] or NULL; may be dh */
    float *dgx;              /* [N][3D] */
    float *dgh;              /* [N][3D] */
    float *dh;               /* [N][D] */
} gnnmp_gru_grad_t;
int gnnmp_gru_pointwise_grad_f32(const gnnmp_gru_grad_t *job, int64_t N, int64_t D, gnnmp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * The graph-convolutional recurrent cells (csrc/poly_conv.hip, csrc/recurrent.hip) — what GConvGRUCell, GConvLSTMCell and DCGRUCell
 * (GraphNeuralNetworks/src/layers/temporalconv.jl:237-254, :416-437, :564-575) need beyond the existing exports: the hop on PANELS and the
 * fused gate kernels, forward and pullback.  A step of a cell is: the Chebyshev / diffusion basis of the state written by the hop
 * straight into the column blocks of one panel [N][B D]; ONE gnnmp_dense_f32 over the panel with the gate-stacked weights; one gate
 * kernel, which writes the next state (or r .* h) into block 0 of the panel that is read next.
 *
 *   gnnmp_poly_hop_ld_f32   gnnmp_poly_hop_f32 with a row stride (in floats) for each of z, self, prev, add and out: the SAME kernel
 *                        template, the arithmetic above in the same order, rounded the same way — with every stride = D it has
 *                        gnnmp_poly_hop_f32's bits.  Row i of an operand starts at ptr + i * ld; D floats of it are used.
 *                          - every stride of a given pointer is at least D (ld_z and ld_out always);
 *                          - operands may be column blocks of one allocation; two distinct blocks of one panel do not overlap;
 *                          - out MAY BE prev OR add, with the same pointer AND the same stride; out may NOT overlap z or self (nor
 *                            prev or add in any other way).  Overlap of two blocks with equal strides is decided exactly (their byte
 *                            spans meet and their column ranges inside a row meet); with different strides, by their byte spans;
 *                          - lanes are 16 / 8 bytes wide only when D % 4 / D % 2 == 0 and EVERY given pointer and EVERY given stride
 *                            (in bytes) is a multiple of 16 / 8; 4-byte lanes otherwise.
 *                        Refused before any HIP call (GNNMP_EINVAL, "poly_hop_ld: ..."): everything gnnmp_poly_hop_f32 refuses, a stride
 *                        below D (or above 2^40), the overlaps above.  n_dst = 0 returns GNNMP_OK.
 *
 *   The GRU cell (GConvGRU and DCGRU: `(1 .- z) .* h~ .+ z .* h` and `z .* h + (1 .- z) .* c` are one expression up to a commuted sum).
 *   Gate order (r, z, c).  P [N][T][3D]: the x-side pre-activations of all steps with all biases; a: the state-side product of THIS
 *   step, contiguous — [N][2D] in phase 0, [N][D] in phase 1; h: the state that entered the step, row stride ldh (0: one vector for every
 *   node; NULL: zeros).  Every product and every sum rounded on its own; σ(x) = (t = expf(-|x|); x >= 0 ? 1 / (1 + t) : t / (1 + t)),
 *   tanh = tanhf, as gnnmp_gru_pointwise_f32.
 *   gnnmp_gru_cell_f32      phase 0:  r = σ(P_r[t] + a_r),  z = σ(P_z[t] + a_z)  -> gates[t] (slots r, z)
 *                                     hout = r h                                   (row stride ldhout)
 *                           phase 1:  c = tanhf(P_c[t] + a_c)                      -> gates[t] (slot c);  z is read from gates[t]
 *                                     h' = (1 - z) c + z h                         -> y[n][t], and hout when it is given
 *                           hout is written `rep` (1 or 2) times side by side: hout[n ldhout + j D + d], j < rep — DConv reads the state
 *                           with two weight slices (one a direction), so its panel holds the state in blocks 0 AND 1.
 *   gnnmp_gru_cell_grad_f32 phase 1:  Δ = dy[t] + carry + Σ_{j < rep} carry2_j     (carry [N][D] and carry2, row stride ldc2, nullable)
 *                                     dc_pre = (Δ (1 - z)) (1 - c c)               -> dP[t] slot c and dac [N][D]
 *                                     dz_pre = (Δ (h - c)) (z (1 - z))             -> dP[t] slot z and darz[:, D:2D]
 *                                     part   = Δ z                                 -> part [N][D]
 *                           phase 0:  q = Σ_{j < rep} drh_j                        (drh: row stride lddrh; the panel cotangent's block 0)
 *                                     dr_pre = (q h) (r (1 - r))                   -> dP[t] slot r and darz[:, 0:D]
 *                                     part   = part + q r
 *                           dac [N][D] and darz [N][2D] are contiguous: what the next dense adjoint reads.  The cotangent of h is
 *                           part + (block 0 of the cotangent of the phase-0 panel): the next (earlier) step takes the two as carry, carry2.
 *
 *   The peephole LSTM cell (GConvLSTM).  Gate order (i, f, c, o); w [4][D] the peepholes; P [N][T][4D]; a [N][4D]; c: the cell state
 *   that entered, row stride ldc (0: one vector; NULL: zeros).
 *   gnnmp_lstm_cell_f32       i = σ(P_i + a_i + w_i c),  f = σ(P_f + a_f + w_f c),  g = tanhf(P_c + a_c + w_c c),  c' = f c + i g,
 *                             o = σ(P_o + a_o + w_o c'),  h' = o tanhf(c');   (P + a first, then + w c)
 *                             gates[t] = (i, f, g, o) and cnew[n][t] = c' are kept for the pullback; h' -> y[n][t] and hout (row
 *                             stride ldhout) when given.
 *   gnnmp_lstm_cell_grad_f32  Δh = dy[t] + carry_h (row stride ldch; nullable),  th = tanhf(c')
 *                             do_pre = (Δh th) (o (1 - o))
 *                             Δc'    = (Δh o) (1 - th th) + carry_c + do_pre w_o          (carry_c [N][D], nullable)
 *                             di_pre = (Δc' g) (i (1 - i)),  df_pre = (Δc' c) (f (1 - f)),  dg_pre = (Δc' i) (1 - g g)
 *                             Δc     = Δc' f + di_pre w_i + df_pre w_f + dg_pre w_c        -> dc [N][D]
 *                             (di, df, dg, do)_pre -> dP[t] and da [N][4D]; peep [N][T][4D] (nullable) gets (di_pre c, df_pre c,
 *                             dg_pre c, do_pre c') at [t]: its column sums over all N T rows are the peepholes' gradients.
 *
 *   job    const HOST records of device pointers, strides and counts (below).  Outputs must not overlap inputs or each other.
 *   N, T, t, D   N >= 0 (N = 0 launches nothing), 1 <= T <= 2^20, 0 <= t < T, N T <= 2^40, 1 <= D <= 2^20; one thread an element.
 * All of them only launch on `stream`: no atomics, every output element written once by one lane, no allocation, no host wait, no
 * scratch; each may be recorded into a HIP graph without an eager call first; two calls give equal bits.
 * Refused before any HIP call (GNNMP_EINVAL), by name ("gru_cell: ...", "gru_cell_grad: ...", "lstm_cell: ...", "lstm_cell_grad: ..."): a
 * NULL job; a phase other than 0 / 1; N, T, t, D outside their ranges; a NULL required pointer (gru_cell: P, a, gates, hout in phase 0, y
 * in phase 1; gru_cell_grad: gates, dP, darz, part, dy and dac in phase 1, drh in phase 0; lstm_cell: P, a, w, gates, cnew, y;
 * lstm_cell_grad: dy, gates, w, cnew, dP, da, dc); a state stride that is neither 0 nor at least D; rep outside {1, 2}; an output or
 * addend stride below rep D (ldhout, ldc2, lddrh) or D (the LSTM's ldhout, ldch).
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
    const float *z;          /* [n_src] rows of D, stride ld_z */
    const float *w_slot;     /* [n_total], plan slot order, or NULL */
    const float *ss_slot;    /* [n_total], plan slot order, or NULL */
    const float *scale_dst;  /* [n_dst] or NULL */
    const float *self;       /* [n_dst] rows of D, stride ld_self, or NULL */
    const float *prev;       /* [n_dst] rows of D, stride ld_prev, or NULL; may be out (same stride) */
    const float *add;        /* [n_dst] rows of D, stride ld_add, or NULL; may be out (same stride) */
    float alpha, beta, gamma;
    float *out;              /* [n_dst] rows of D, stride ld_out */
    int64_t ld_z, ld_self, ld_prev, ld_add, ld_out;      /* row strides in floats; those of NULL operands are not read */
} gnnmp_poly_hop_ld_t;
int gnnmp_poly_hop_ld_f32(const gnnmp_graph_t *plan, const gnnmp_poly_hop_ld_t *job, int64_t D, gnnmp_stream_t stream);

typedef struct {
    const float *P;          /* [N][T][3D] */
    const float *a;          /* phase 0: [N][2D] (r, z); phase 1: [N][D] */
    const float *h;          /* rows of D, stride ldh (0: one vector), or NULL (zeros) */
    int64_t ldh;
    float *gates;            /* [N][T][3D]: phase 0 writes r, z of step t; phase 1 reads z and writes c */
    float *hout;             /* rows of rep D, stride ldhout; phase 1: or NULL */
    int64_t ldhout;
    int rep;                 /* 1 or 2 */
    float *y;                /* [N][T][D], phase 1 */
} gnnmp_gru_cell_t;
int gnnmp_gru_cell_f32(int phase, const gnnmp_gru_cell_t *job, int64_t N, int64_t T, int64_t t, int64_t D, gnnmp_stream_t stream);

typedef struct {
    const float *dy;         /* [N][T][D], phase 1 */
    const float *carry;      /* [N][D] or NULL, phase 1 */
    const float *carry2;     /* rows of rep D, stride ldc2, or NULL, phase 1 */
    int64_t ldc2;
    const float *gates;      /* [N][T][3D] */
    const float *h;          /* as in the forward */
    int64_t ldh;
    const float *drh;        /* rows of rep D, stride lddrh, phase 0 */
    int64_t lddrh;
    int rep;                 /* 1 or 2 */
    float *dP;               /* [N][T][3D]: step t written (c, z in phase 1; r in phase 0) */
    float *dac;              /* [N][D], phase 1 */
    float *darz;             /* [N][2D]: z half in phase 1, r half in phase 0 */
    float *part;             /* [N][D]: written in phase 1, updated in phase 0 */
} gnnmp_gru_cell_grad_t;
int gnnmp_gru_cell_grad_f32(int phase, const gnnmp_gru_cell_grad_t *job, int64_t N, int64_t T, int64_t t, int64_t D,
                            gnnmp_stream_t stream);

typedef struct {
    const float *P;          /* [N][T][4D] */
    const float *a;          /* [N][4D] */
    const float *w;          /* [4][D] */
    const float *c;          /* rows of D, stride ldc (0: one vector), or NULL (zeros) */
    int64_t ldc;
    float *gates;            /* [N][T][4D]: step t written */
    float *cnew;             /* [N][T][D]: step t written */
    float *hout;             /* rows of D, stride ldhout, or NULL */
    int64_t ldhout;
    float *y;                /* [N][T][D]: step t written */
} gnnmp_lstm_cell_t;
int gnnmp_lstm_cell_f32(const gnnmp_lstm_cell_t *job, int64_t N, int64_t T, int64_t t, int64_t D, gnnmp_stream_t stream);

typedef struct {
    const float *dy;         /* [N][T][D] */
    const float *carry_h;    /* rows of D, stride ldch, or NULL */
    int64_t ldch;
    const float *carry_c;    /* [N][D] or NULL */
    const float *gates;      /* [N][T][4D] */
    const float *w;          /* [4][D] */
    const float *c;          /* as in the forward */
    int64_t ldc;
    const float *cnew;       /* [N][T][D] */
    float *dP;               /* [N][T][4D]: step t written */
    float *da;               /* [N][4D] */
    float *dc;               /* [N][D] */
    float *peep;             /* [N][T][4D] or NULL: step t written */
} gnnmp_lstm_cell_grad_t;
int gnnmp_lstm_cell_grad_f32(const gnnmp_lstm_cell_grad_t *job, int64_t N, int64_t T, int64_t t, int64_t D, gnnmp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Float64 features (round 6).  The reference's message passing is eltype-generic, and its own micro-benchmark runs in Float64
 * (GraphNeuralNetworks/perf/bench_gnn.jl:9-10: `B = rand(100, n)`; it asserts isequal(propagate(e_mul_xj, g, +; xj = B, e), B * A)).  The
 * seam's methods and their leaves exist for `double` too — the same plan, the same walk, the same order of operations as the `_f32` entry
 * points (adds in ORIGINAL edge order, products rounded separately: bit-identical to NNlib's CPU loop on every row the plan does not split;
 * split rows: chunk partials folded in chunk order, deterministic):
 *   gnnmp_propagate_f64   propagate(copy_xj | w_mul_xj | e_mul_xj with a vector e, g, + | mean | max | min)   msgpass.jl:71-79, 215-238;
 *                         arguments as gnnmp_propagate_f32 (w: n_edges doubles in original edge order; scale_src / scale_dst nullable)
 *   gnnmp_gather_f64      _gather   (gatherscatter.jl:4)
 *   gnnmp_scatter_f64     _scatter  (gatherscatter.jl:12-18) with idx = the plan's targets, m in original edge order
 * The layer bodies' dense products stay with the caller in Float64 (`l.weight * x` is rocBLAS in Julia): the fused layer kernels, the
 * attention kernels and the adjoints are Float32 only, and so is everything `bench.py` measures.
 * ---------------------------------------------------------------------------------------------- */
int gnnmp_propagate_f64(gnnmp_graph_t *plan, int msg, int aggr, const double *xj, const double *w, const double *scale_src,
                        const double *scale_dst, double *out, int64_t D, gnnmp_stream_t stream);
int gnnmp_gather_f64(const double *x, const void *idx, int idx_bytes, int index_base, int64_t K, double *out, int64_t D,
                     gnnmp_stream_t stream);
int gnnmp_scatter_f64(gnnmp_graph_t *plan, int aggr, const double *m, double *out, int64_t D, gnnmp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Repair hook.  The split rows of a plan are folded inside the row kernels through per-plan arrival counters that every launch leaves at
 * zero (csrc/common.h: ensure_arrive states the invariant and when it holds).  A caller that broke the one-stream-per-plan rule above
 * — two compute calls on one plan in flight at once — may leave them dirty, and every later result on that plan's split rows would be
 * wrong.  gnnmp_plan_reset_counters enqueues a memset of the counters (and of the fused layer kernel's tile ticket) on `stream`; a few
 * KB, no synchronisation, a no-op for a plan without split rows.  Never needed by a caller that keeps the rule.
 * ---------------------------------------------------------------------------------------------- */
int gnnmp_plan_reset_counters(gnnmp_graph_t *plan, gnnmp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Flux.LSTMCell at batch one on a long vector: the recurrence of EvolveGCNOCell (GraphNeuralNetworks/src/layers/temporalconv.jl:678-705),
 * whose LSTM evolves the FLATTENED convolution weight — D = in * out, Wi and Wh [4D][D] row-major (Julia (4D, D) read row by row: the
 * caller's [4D, D] tensors), gate order (input, forget, cell, output), b [4D].  A step is two matrix-vector products that read 8 D^2
 * floats; csrc/evolve.hip.  σ(x) = (t = expf(-|x|); x >= 0 ? 1 / (1 + t) : t / (1 + t)), tanh = tanhf, as gnnmp_lstm_pointwise_f32;
 * every product and every sum is rounded on its own.
 *   gnnmp_lstm_matvec_cell_f32         one whole step:  a = Wi x + Wh h + b,  c' = σ(a_f) c + σ(a_i) tanhf(a_c),  h' = σ(a_o) tanhf(c').
 *                                      gnnmp_lstm_matvec_t: Wi, x read; Wh and h [D] read, or h NULL (zeros: the Wh product is skipped and
 *                                      Wh is not read); c [D] or NULL (zeros); b [4D] or NULL; h_out [D], c_out [D] written; a_out [4D]
 *                                      (the pre-activations, bias included: what the pullback recomputes the gates from) written, or NULL.
 *                                      x and h may be the same array.  A lane group owns element j and streams the rows j, D + j, 2D + j,
 *                                      3D + j of both matrices: a_j is the sum of the lanes' partials (each over the columns f, f + G VEC,
 *                                      ... ascending, the Wi terms of a pass before its Wh terms) folded by an xor butterfly, + b.  The
 *                                      group is up to a wave; for D <= 2048 a row that fills 256 lanes goes to a whole workgroup, whose
 *                                      four waves' sums are added in wave order (one wave an element would be too few waves).  Lanes
 *                                      are 16 / 8 bytes wide only when D % 4 / D % 2 == 0 and Wi, Wh, x, h are aligned to as much.
 *                                      Refused (GNNMP_EINVAL, "lstm_matvec_cell: ..."): a NULL job; D outside 0 .. 2^20; NULL Wi, x, h_out
 *                                      or c_out; h without Wh; an output that overlaps x, h or c (other workgroups still read them) or
 *                                      another output.  D = 0 returns GNNMP_OK.
 *   gnnmp_lstm_matvec_grad_workspace   floats of scratch gnnmp_lstm_matvec_grad_f32 needs at D: a pure host function (0 for a D outside
 *                                      1 .. 2^20)
 *   gnnmp_lstm_matvec_grad_f32         the transposed products:  out_x = Wi' da (+ add_x),  out_h = Wh' da (+ add_h); either output may
 *                                      be NULL (its matrix is then not read).  sum = 1:  out_x = (Wi' da + Wh' da) + add_x — from the
 *                                      second step on the LSTM's input and its hidden state are one array (out_h and add_h must be
 *                                      NULL).  gnnmp_lstm_matvec_grad_t: da [4D]; add_x, add_h [D] or NULL; ws, ws_floats the scratch.
 *                                      Each matrix is read once, rows coalesced; its 4D rows are cut into slabs whose partial sums (rows
 *                                      ascending) go to ws, and a SECOND LAUNCH adds the slabs in ascending order: no workgroup waits
 *                                      on another, equal bits from call to call.  Refused (GNNMP_EINVAL, "lstm_matvec_grad: ..."): a NULL
 *                                      job; D outside 0 .. 2^20; sum outside {0, 1}; NULL da; both outputs NULL; a wanted matrix NULL; an
 *                                      addend without its output; out_h or add_h with sum = 1; a NULL or short workspace; an output that
 *                                      overlaps da, the workspace or the other output; a workspace that overlaps da or an addend.  D = 0
 *                                      returns GNNMP_OK.
 *   gnnmp_outer_accum_f32              the rank-T update:  dW[r][k] = Σ_t A[t][r] B[t][k], t ascending, from zero; dW [R][K] written once;
 *                                      db[r] = Σ_t A[t][r] when db is given.  gnnmp_outer_accum_t: A [T][R], B [T][K] read; dW, db or NULL
 *                                      written.  ΔWi = (A = the steps' da, B = the steps' inputs), ΔWh = (B = the hidden states that entered).
 *                                      Write-bound: whole 16-byte lanes side by side when K % 4 == 0 and B, dW are aligned.  Refused
 *                                      (GNNMP_EINVAL, "outer_accum: ..."): a NULL job; T outside 0 .. 2^20, R outside 0 .. 2^22, K outside
 *                                      0 .. 2^20; NULL A, B or dW; an output that overlaps an input or the other output.  T = 0 (the empty
 *                                      sum), R = 0, or K = 0 without db: GNNMP_OK, nothing is launched and NOTHING IS WRITTEN.
 *   job    const HOST records of device pointers and scalars (below).
 * All three compute calls only launch on `stream`: no atomics, no allocation, no host wait, nothing owned by a plan; each may be recorded
 * into a HIP graph without an eager call first; two calls give equal bits.  Element offsets are 64-bit (4D * D passes 2^31 at D = 23 171).
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
    const float *Wi;         /* [4D][D] */
    const float *Wh;         /* [4D][D]; may be NULL when h is */
    const float *x;          /* [D] */
    const float *h;          /* [D] or NULL (zeros) */
    const float *c;          /* [D] or NULL (zeros) */
    const float *b;          /* [4D] or NULL */
    float *h_out;            /* [D] */
    float *c_out;            /* [D] */
    float *a_out;            /* [4D] or NULL */
} gnnmp_lstm_matvec_t;
int gnnmp_lstm_matvec_cell_f32(const gnnmp_lstm_matvec_t *job, int64_t D, gnnmp_stream_t stream);

typedef struct {
    const float *Wi;         /* [4D][D]; read when out_x is given */
    const float *Wh;         /* [4D][D]; read when out_h is given or sum = 1 */
    const float *da;         /* [4D] */
    const float *add_x;      /* [D] or NULL */
    const float *add_h;      /* [D] or NULL */
    float *out_x;            /* [D] or NULL */
    float *out_h;            /* [D] or NULL */
    int sum;                 /* 1: out_x = Wi' da + Wh' da + add_x */
    float *ws;               /* ws_floats >= gnnmp_lstm_matvec_grad_workspace(D) floats of scratch */
    int64_t ws_floats;
} gnnmp_lstm_matvec_grad_t;
int64_t gnnmp_lstm_matvec_grad_workspace(int64_t D);
int gnnmp_lstm_matvec_grad_f32(const gnnmp_lstm_matvec_grad_t *job, int64_t D, gnnmp_stream_t stream);

typedef struct {
    const float *A;          /* [T][R] */
    const float *B;          /* [T][K] */
    float *dW;               /* [R][K] */
    float *db;               /* [R] or NULL */
} gnnmp_outer_accum_t;
int gnnmp_outer_accum_f32(const gnnmp_outer_accum_t *job, int64_t T, int64_t R, int64_t K, gnnmp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * TopKPool and topk_index (csrc/topk.hip) — GraphNeuralNetworks/src/layers/pool.jl (TopKPool), GNNlib/src/layers/pool.jl:14-27
 * (topk_pool, topk_index):
 *     y = p' * X / norm(p);  idx = topk_index(y, k);  A~ = view(A, idx, idx);  X_ = view(X, :, idx) .* σ.(view(y, idx)')
 * The reference pools one graph held as a dense matrix.  Here the unit is a batch: selection is per member graph, the child graph's plan
 * comes from gnnmp_plan_keep_nodes (above) with the keep flags of the selection, and the gate and its pullback are row kernels.  Float32,
 * device pointers, the caller owns every array.  The four calls of this section only launch on `stream`: no host wait, nothing taken
 * from a pool, no atomics; each may be recorded into a HIP graph without an eager call first; two calls give equal bits.
 *
 * The row kernels give a row of C floats L lanes, L = the power of two >= min(C, 64): lane l adds the channels c = l, l + L, l + 2L, ...
 * in ascending order, each product rounded before it is added, and the L partial sums fold in a butterfly (lane ^ L/2, ..., lane ^ 1).
 * This is "the association of the row sum" wherever a row sum is spoken of below; norm(p) = sqrtf of the row sum of p[c] * p[c].
 * Any C >= 1 works (a row wider than the lanes is walked in strides); 4-byte alignment is all a pointer owes.
 *
 * The ORDER of a selection.  key(v) = the monotone map of the fp32 bits to uint32 (b ^ 0xffffffff for a set sign bit, b | 0x80000000
 * otherwise) after -0.0 is replaced by +0.0; every NaN has key 0, below -Inf.  Inside its member graph, node i has
 *     rank_i = #{ j : key_j > key_i } + #{ j < i : key_j == key_i }
 * — larger scores first, equal keys by ascending node id, NaNs after every number and among themselves by id.  A member graph of n_g
 * nodes has k_g = min(n_g, k), or with k == 0  k_g = min(n_g, (int64) ceil((double) ratio * (double) n_g)).
 *     ties = GNNMP_TOPK_TIES_FIRST (the layer)     keep[i] = rank_i < k_g: exactly k_g nodes
 *     ties = GNNMP_TOPK_TIES_ALL (topk_index)      keep[i] = #{ j : key_j > key_i } < k_g: every node whose key is at least the key of rank
 *                                                  k_g - 1; more than k_g of them when equal keys straddle that rank
 * An empty member graph keeps nothing and is no error.  Integer work only: the result is exact and the same on both routes.
 * ---------------------------------------------------------------------------------------------- */
#define GNNMP_TOPK_TIES_FIRST 0
#define GNNMP_TOPK_TIES_ALL 1
#define GNNMP_TOPK_ACT_SIGMOID 0
#define GNNMP_TOPK_ACT_TANH 1
#define GNNMP_TOPK_ACT_IDENTITY 2
#define GNNMP_TOPK_GRAD_ROWS 64

/* y[i] = (sum_c p[c] * x[i][c]) / norm(p) for x [N][C] row-major, p [C], y [N]  (pool.jl:15).  The row sum and norm(p) in the association
 * stated above; norm(p) is computed inside the kernel from p on the device (no host read of p).  norm(p) = 0 gives what IEEE division
 * gives (NaN or an infinity), as in the reference.  Refused (GNNMP_EINVAL, before any launch): N < 0, C < 1, p NULL, x or y NULL with
 * N > 0; N >= 2^31 - 1: GNNMP_EUNSUPPORTED.  N = 0: GNNMP_OK, nothing is launched. */
int gnnmp_topk_score_f32(const float *x, const float *p, float *y, int64_t N, int64_t C, gnnmp_stream_t stream);

/* The selection: keep flags (and ranks) of the N nodes of a batch from their scores, in the order stated above.
 *   score             [N]
 *   graph_ptr         [n_graphs + 1] 0-based node offsets of the member graphs (idx_bytes 4 | 8; empty graphs allowed), or NULL: one graph.
 *                     It must ascend from 0 to N.  This is NOT checked (a check would need a host wait); the Python layer passes the
 *                     array gnnmp_segment_bounds wrote.  With another array the result is undefined, but nothing outside the arrays of the
 *                     call is read or written.
 *   k, ratio          k >= 1: a fixed k; k == 0: ratio in (0, 1] (a float: k_g is taken from ITS value, so (float) 0.1 of 30 nodes
 *                     is ceil(3.0000000447) = 4)
 *   ties              GNNMP_TOPK_TIES_FIRST | GNNMP_TOPK_TIES_ALL
 *   lds_budget_bytes  0 = the default (1 KB = 256 keys); values above 64 KB count as 64 KB, values below 4 as 4.  A member graph whose
 *                     keys fit takes the LDS route: the workgroup that owns the 256-node tile a graph STARTS in loads the keys of a run
 *                     of consecutive such graphs into LDS (as many as fit the budget) and gives every node one thread.  A larger member
 *                     graph takes the device-memory route: n_g / 256 workgroups, each streaming the graph's keys from device memory.
 *                     The result does not depend on the budget.
 *   keep              uint32 [N + 1]: 1 | 0 per node, keep[N] = 0 — the form gnnmp_plan_keep_nodes and its scan consume.  All written.
 *   rank              int32 [N] or NULL: rank_i, 0-based inside the member graph.  All written.
 * Needs no scratch.  Refused (GNNMP_EINVAL, before any launch, nothing written): job or keep NULL, score NULL with N > 0, N < 0,
 * idx_bytes not 4 | 8, n_graphs < 1 with a graph_ptr, k < 0, k == 0 with a ratio outside (0, 1] (a NaN included), a ties value other
 * than the two, a negative lds_budget_bytes; N >= 2^31 - 1: GNNMP_EUNSUPPORTED. */
typedef struct {
    const float *score;
    const void *graph_ptr;
    int idx_bytes;
    int64_t n_graphs;
    int64_t k;
    float ratio;
    int ties;
    int64_t lds_budget_bytes;
    uint32_t *keep;
    int32_t *rank;
} gnnmp_topk_t;
int gnnmp_topk_select_f32(const gnnmp_topk_t *job, int64_t N, gnnmp_stream_t stream);

/* out[r][:] = x[node_map[r]][:] * act(y[node_map[r]]) for r < n_keep  (pool.jl:25): gather and gate in one pass.
 *   x [N][C], y [N], node_map int32 [n_keep] (0-based parent ids: gnnmp_plan_keep_nodes' node_map_out; not range-checked),
 *   act GNNMP_TOPK_ACT_SIGMOID (the reference: 1 / (1 + expf(-y))) | _TANH (tanhf) | _IDENTITY, out [n_keep][C], all written.
 * Refused (GNNMP_EINVAL, before any launch): job NULL, n_keep < 0, C < 1, another act, a NULL array with n_keep > 0.  n_keep = 0: GNNMP_OK,
 * nothing is launched. */
typedef struct {
    const float *x;
    const float *y;
    const int32_t *node_map;
    int act;
    float *out;
} gnnmp_topk_gate_t;
int gnnmp_topk_gate_f32(const gnnmp_topk_gate_t *job, int64_t n_keep, int64_t C, gnnmp_stream_t stream);

/* The pullback of score + gate in ONE walk over the parent's N rows.  With r = node_new[i] (int32 [N], -1 for a dropped node:
 * gnnmp_plan_keep_nodes' node_new_out), g = act(y_i) and dout [n_keep][C] the cotangent of out:
 *     dy_i    = act'(y_i) * sum_c dout[r][c] * x[i][c]                 (the row sum in the association stated above; 0 for a dropped node)
 *     dx[i][c] = dout[r][c] * g + (dy_i * p[c]) / norm(p)              (p == NULL — an externally supplied score: the first term alone);
 *                                                                       a dropped node's row is ZERO; dx [N][C] is written whole
 *     dp[c]   = (sum_i dy_i * x[i][c]) / norm(p) - ((sum_i dy_i * y_i) * p[c]) / norm(p)^2
 * dy [N] (optional, NULL to skip) and dp [C] (optional; needs p and part) are written whole.  The two sums over nodes are folded in two
 * fixed stages: workgroup b adds the kept rows b * GNNMP_TOPK_GRAD_ROWS .. in ascending i into part[b][0 .. C] (column C: dy_i * y_i),
 * then one launch adds the workgroups in ascending b — no float atomics, equal bits from call to call.  No gradient flows through the
 * selection (it is piecewise constant).
 *   part   caller scratch, ceil(N / GNNMP_TOPK_GRAD_ROWS) * (C + 1) floats; read and written only when dp is given
 * Refused (GNNMP_EINVAL, before any launch): job NULL, N < 0, C < 1, another act, dp without p or without part, a NULL x, y, dout,
 * node_new or dx with N > 0.  N = 0: GNNMP_OK; dp (when given) is written as zeros. */
typedef struct {
    const float *x;
    const float *y;
    const float *p;
    const float *dout;
    const int32_t *node_new;
    int act;
    float *dx;
    float *dy;
    float *dp;
    float *part;
} gnnmp_topk_gate_grad_t;
int gnnmp_topk_gate_grad_f32(const gnnmp_topk_gate_grad_t *job, int64_t N, int64_t C, gnnmp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * GNNMP_INTERNAL — exported, NOT part of the drop-in surface: experiment and test hooks.  Declared here so that C callers (tests/c_harness)
 * do not declare them by hand; a Julia / C host has no reason to call them, and their meaning may change between builds.
 *   gnnmp_tune(knob, value)        process-global tuning knobs of the perf experiments (csrc/knobs.h: the table of indices, defaults and
 *                                  meanings).  In the release build every accepted value selects correct code: the one knob whose values
 *                                  compute garbage on purpose (13, phase ablations) is refused with GNNMP_EUNSUPPORTED unless it is 0; only
 *                                  a library built with -DGNNMP_EXPERIMENTS (make EXPERIMENTS=1) takes it.  GNNMP_EINVAL for a bad index.
 *                                  Not thread-safe against concurrent compute calls.
 *   gnnmp_tune_get(knob, &v, &d)   the knob's current value and its default; either pointer may be NULL.  GNNMP_EINVAL for a bad index.
 *   gnnmp_debug_mock_device(d)     d >= 0: the calling thread's "current device" for the library's per-device tables; d < 0: hipGetDevice
 *   gnnmp_debug_device_once(...)   runs the once-per-device machinery with a counting stand-in (tests/test_multi_device_cpu.py)
 *   gnnmp_debug_plan_block(plan)   the pooled block of a gnnmp_plan_concat / gnnmp_plan_select plan (NULL otherwise)
 *   gnnmp_debug_pool_pick(...)     the block pool's slot choice on host arrays
 *   gnnmp_debug_random_walk_pe_f32(...)  gnnmp_random_walk_pe_f32 with the LDS budget of a workgroup in bytes (0 = the default, 64 KB): a
 *                                  small budget sends small graphs through the scratch path (tests/test_rwpe.py)
 *   gnnmp_debug_dense_route(info)  what the last gnnmp_dense_f32 call of the calling thread launched (host memory, written by that
 *                                  call: no synchronisation, no allocation, nothing a stream capture sees).  info[0] = the kernel: 0 none
 *                                  (the call returned before a launch), 1 dense_split, 2 dense_wreg, 3 dense_t16, 4 dense_narrow,
 *                                  5 dense_wlds, 6 dense_mfma.  For dense_wlds: info[1] = column tile (128 | 64), [2] = waves a block
 *                                  (8 | 4), [3] = ks, the columns of x staged per k-chunk, [4] = tp, the column tiles per epilogue pass,
 *                                  [5] = NT of the remainder launch (0 = none), [6] = 1 if the cross-tile prefetch condition held,
 *                                  [7] = column tiles of the full launch (0 = remainder launch only).  Zero for the other kernels.
 *                                  (tests/test_dense_fallbacks.py)
 * ---------------------------------------------------------------------------------------------- */
int gnnmp_tune(int knob, int value);
int gnnmp_tune_get(int knob, int *value, int *default_value);
int gnnmp_debug_mock_device(int dev);
int gnnmp_debug_device_once(const int *devs, int n, int fail_on, int *n_failed);
void *gnnmp_debug_plan_block(const gnnmp_graph_t *plan);
int gnnmp_debug_pool_pick(const uint64_t *caps, int n, uint64_t bytes);
int gnnmp_debug_random_walk_pe_f32(gnnmp_graph_t *plan_t, const gnnmp_rwpe_t *job, int64_t lds_budget_bytes, gnnmp_stream_t stream);
int gnnmp_debug_dense_route(int info[8]);

#ifdef __cplusplus
}
#endif
#endif /* GNNMP_H */
