// hetero.hip — the aggregation of a heterogeneous layer in ONE launch: a destination row is finished over ALL of its incoming relations
// before it is stored.  HeteroGraphConv (GraphNeuralNetworks/src/layers/heteroconv.jl:57-86) runs one layer per relation and folds the
// outputs per destination type, `foldl(aggr, outs)`: composed from propagate that is R launches, R aggregate matrices written and
// R - 1 passes to add them — every aggregate row, 4 D bytes, written once and read once for nothing.  Here:
//   - one GROUP of G = 2^k lanes (16 bytes a lane, as in csr_rows_kernel) owns one destination row of one destination type;
//   - it walks the row in each incoming relation in turn with reduce_range (csr_reduce.h): ORIGINAL edge order, 8 row loads in flight,
//     and finishes the relation's aggregate as finalize_row does (mean's division; an empty row keeps the operator's identity);
//   - the aggregate is folded into a running value in registers, in table order: out[i] = foldl(⊕, m_1[i], ..., m_R[i]);
//   - one store per row.  One launch covers every destination type of the layer: blocks [blk_end[d-1], blk_end[d]) belong to type d.
// A relation without a plan is an IDENTITY relation: it contributes row i of an [n_dst][D] matrix as it is — a layer's root term, or
// a finished layer output when the kernel is used as the combiner of R outputs.
// A row longer than its plan's split threshold is walked whole by its lane group (correct, in edge order, slow for hubs: the host
// layer sends graphs with split rows to the composition, gnnmp/hetero.py).  Nothing here touches a plan's workspace: the tables
// travel by value in the kernel arguments, the export neither allocates nor synchronises.
//
// The operator differs per relation at run time.  It is a switch around the walk (uniform per block: all lane groups of a block
// belong to one destination type), not one launch per operator class: the running value lives in registers across relations of
// different operators, and the three inlined walks cost no registers beyond the widest one (DESIGN.md §3 has the figures).
#include "csr_reduce.h"

namespace gnnmp {

struct HeteroRel {              // what the whole-row walk reads of a relation's PlanRows; rowptr == null: identity relation
    const uint32_t *rowptr;
    const int32_t *col, *eid;
    const float *x;             // [n_src][D]; identity: [n_dst][D]
    const float *w;             // [n_edges] original order, nullable (the w_mul_xj message)
    uint32_t n_edges;
    int aggr;                   // gnnmp_aggr
};
struct HeteroDst {
    float *out;                 // [n_dst][D]
    int n_dst;
    int combine;                // OP_SUM | OP_MAX | OP_MIN
    int rel_beg, rel_end;       // its relations in HeteroArgs::rel, in fold order
    uint32_t blk_end;           // one past its last block (prefix of block counts)
};
struct HeteroArgs {
    HeteroDst dst[GNNMP_HETERO_MAX_REL];
    HeteroRel rel[GNNMP_HETERO_MAX_REL];
    int n_dsts, D, log2g, waves;
};

template <int VEC, int OP, bool SCALED>
__device__ __forceinline__ void hetero_walk(const HeteroRel &r, int D, int row, int lig, int gbase, int G, int f0, bool active,
                                            float acc[VEC]) {
    ReduceArgs a = {};
    a.rows.col = r.col;
    a.rows.eid = r.eid;
    a.rows.n_edges = r.n_edges;
    a.x = r.x;
    a.w = r.w;
    a.D = D;
    a.mean = r.aggr == GNNMP_MEAN;
    const uint32_t beg = r.rowptr[row], end = r.rowptr[row + 1];
#pragma unroll
    for (int q = 0; q < VEC; ++q) acc[q] = op_identity<OP>();
    reduce_range<VEC, OP, SCALED, 8>(a, beg, end, lig, gbase, G, f0, active, acc);
    finalize_row<VEC, OP>(a, row, end - beg, acc);
}

template <int VEC, int OP>
__device__ __forceinline__ void hetero_fold(float run[VEC], const float acc[VEC]) {
#pragma unroll
    for (int q = 0; q < VEC; ++q) run[q] = op_apply<OP>(run[q], acc[q]);
}

// SCALED: some relation of the call carries w (a relation without one multiplies by 1.0f: the same bits)
template <int VEC, bool SCALED>
__global__ void __launch_bounds__(256) hetero_rows_kernel(const HeteroArgs h) {
    int d = 0;
    uint32_t b0 = 0;
    while (d < h.n_dsts - 1 && blockIdx.x >= h.dst[d].blk_end) b0 = h.dst[d++].blk_end;
    const HeteroDst &dd = h.dst[d];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int G = 1 << h.log2g;
    const int lig = lane & (G - 1), gbase = lane - lig;
    const int64_t row64 = ((int64_t)(blockIdx.x - b0) * h.waves + wave) * (64 >> h.log2g) + (lane >> h.log2g);
    if (row64 >= dd.n_dst) return;
    const int row = (int)row64;
    const int f0 = ((int)blockIdx.y * G + lig) * VEC;
    const bool active = f0 < h.D;
    float run[VEC];
#pragma unroll
    for (int q = 0; q < VEC; ++q) run[q] = 0.0f;
    for (int k = dd.rel_beg; k < dd.rel_end; ++k) {
        const HeteroRel &r = h.rel[k];
        float acc[VEC];
        if (!r.rowptr) {
#pragma unroll
            for (int q = 0; q < VEC; ++q) acc[q] = 0.0f;
            if (active) Vec<VEC>::load(r.x + (int64_t)row * h.D + f0, acc);
        } else {
            switch (r.aggr) {
                case GNNMP_MAX: hetero_walk<VEC, OP_MAX, SCALED>(r, h.D, row, lig, gbase, G, f0, active, acc); break;
                case GNNMP_MIN: hetero_walk<VEC, OP_MIN, SCALED>(r, h.D, row, lig, gbase, G, f0, active, acc); break;
                default: hetero_walk<VEC, OP_SUM, SCALED>(r, h.D, row, lig, gbase, G, f0, active, acc); break;
            }
        }
        if (k == dd.rel_beg) {
#pragma unroll
            for (int q = 0; q < VEC; ++q) run[q] = acc[q];
        } else if (dd.combine == OP_MAX) {
            hetero_fold<VEC, OP_MAX>(run, acc);
        } else if (dd.combine == OP_MIN) {
            hetero_fold<VEC, OP_MIN>(run, acc);
        } else {
            hetero_fold<VEC, OP_SUM>(run, acc);
        }
    }
    if (active) Vec<VEC>::store(dd.out + (int64_t)row * h.D + f0, run);
}

}  // namespace gnnmp

using namespace gnnmp;

extern "C" int gnnmp_hetero_propagate_f32(const gnnmp_hetero_dst_t *dsts, int n_dsts, int64_t D, gnnmp_stream_t stream) {
    if (!dsts || n_dsts < 1) return fail(GNNMP_EINVAL, "hetero_propagate: null or empty destination table");
    if (D < 1 || D > (1 << 20)) return fail(GNNMP_EINVAL, "hetero_propagate: bad D %lld", (long long)D);
    int64_t n_rel = 0;
    for (int d = 0; d < n_dsts; ++d) {
        if (dsts[d].n_rel < 1 || !dsts[d].rels) return fail(GNNMP_EINVAL, "hetero_propagate: destination %d has no relation table", d);
        n_rel += dsts[d].n_rel;
    }
    if (n_rel > GNNMP_HETERO_MAX_REL)
        return fail(GNNMP_EUNSUPPORTED, "hetero_propagate: %lld relations in one call (at most %d)", (long long)n_rel, GNNMP_HETERO_MAX_REL);
    HeteroArgs h = {};
    h.n_dsts = n_dsts;
    h.D = (int)D;
    uintptr_t align = 0;
    bool scaled = false;
    int k = 0;
    for (int d = 0; d < n_dsts; ++d) {
        const gnnmp_hetero_dst_t &s = dsts[d];
        if (s.n_dst < 0 || s.n_dst >= INT32_MAX) return fail(GNNMP_EINVAL, "hetero_propagate: destination %d: bad n_dst %lld", d, (long long)s.n_dst);
        if (s.combine != GNNMP_SUM && s.combine != GNNMP_MAX && s.combine != GNNMP_MIN)
            return fail(GNNMP_EINVAL, "hetero_propagate: destination %d: bad combine %d (+, max or min)", d, s.combine);
        if (!s.out && s.n_dst > 0) return fail(GNNMP_EINVAL, "hetero_propagate: destination %d: null out", d);
        HeteroDst &o = h.dst[d];
        o.out = s.out;
        o.n_dst = (int)s.n_dst;
        o.combine = s.combine == GNNMP_MAX ? OP_MAX : (s.combine == GNNMP_MIN ? OP_MIN : OP_SUM);
        o.rel_beg = k;
        align |= reinterpret_cast<uintptr_t>(s.out);
        for (int j = 0; j < s.n_rel; ++j, ++k) {
            const gnnmp_hetero_rel_t &r = s.rels[j];
            HeteroRel &q = h.rel[k];
            const gnnmp_graph_t *p = r.plan;
            if (r.aggr < GNNMP_SUM || r.aggr > GNNMP_MIN) return fail(GNNMP_EINVAL, "hetero_propagate: destination %d relation %d: bad aggr %d", d, j, r.aggr);
            if (p && p->n_dst != s.n_dst)
                return fail(GNNMP_EINVAL, "hetero_propagate: destination %d relation %d: the plan has %lld destinations, the table %lld", d, j,
                            (long long)p->n_dst, (long long)s.n_dst);
            if (!r.x && s.n_dst > 0 && (!p || p->n_total > 0)) return fail(GNNMP_EINVAL, "hetero_propagate: destination %d relation %d: null x", d, j);
            if (p) {
                q.rowptr = p->rowptr;
                q.col = p->col;
                q.eid = p->eid;
                q.n_edges = (uint32_t)p->n_edges;
                q.w = r.w;
                q.aggr = r.aggr;
                scaled = scaled || r.w;
            }
            q.x = r.x;
            align |= reinterpret_cast<uintptr_t>(r.x);
        }
        o.rel_end = k;
    }
    const int vec = pick_vec(D, reinterpret_cast<const void *>(align), nullptr);
    h.log2g = pick_log2g((D + vec - 1) / vec);
    h.waves = 4;
    const int rows_per_block = (64 >> h.log2g) * h.waves;
    int64_t blocks = 0;
    for (int d = 0; d < n_dsts; ++d) {
        blocks += (dsts[d].n_dst + rows_per_block - 1) / rows_per_block;
        if (blocks >= INT32_MAX) return fail(GNNMP_EUNSUPPORTED, "hetero_propagate: too many row blocks");
        h.dst[d].blk_end = (uint32_t)blocks;
    }
    if (blocks == 0) return GNNMP_OK;
    const dim3 grid((unsigned)blocks, (unsigned)feature_tiles(D, vec, h.log2g));
    with_vec(vec, [&](auto V) {
        constexpr int VEC = decltype(V)::value;
        if (scaled)
            hetero_rows_kernel<VEC, true><<<grid, 64 * h.waves, 0, (hipStream_t)stream>>>(h);
        else
            hetero_rows_kernel<VEC, false><<<grid, 64 * h.waves, 0, (hipStream_t)stream>>>(h);
    });
    GNNMP_LAUNCH_CHECK("hetero_rows_kernel");
    return GNNMP_OK;
}
