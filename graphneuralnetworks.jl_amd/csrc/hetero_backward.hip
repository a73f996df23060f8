// hetero_backward.hip — the adjoint of the heterograph aggregation w.r.t. the node features, in ONE launch: a source row is finished over
// ALL the relations that leave it before it is stored.  The backward of hetero.hip has the forward's shape, mirrored: what a source type
// receives is a sum over its outgoing relations.  Composed from the homogeneous adjoints that is, per relation, one transposed propagate
// (or gnnmp_propagate_maxmin_grad_f32), one [n_src][D] matrix written, one pass to add it and — for mean — one pass to pre-scale Δ by
// 1/count.  Here:
//   - one GROUP of G = 2^k lanes owns one source row j of one source type (blocks [blk_end[s-1], blk_end[s]) belong to type s);
//   - it walks row j of each outgoing relation's TRANSPOSED plan in turn (rows = source nodes, col = destination, slots in ORIGINAL edge
//     order) and keeps the running sum in registers, in table order, the first term copied: dx[j] = c_1[j] + ... + c_R[j];
//   - one store per row.
// A relation's term takes one of four modes, decided per relation on the host (uniform per block):
//   LINEAR    adjoint of + / mean, with or without edge weights: c[j] = Σ_p w[eid_p] * (dy[col_p] * sd[col_p]) — reduce_range (csr_reduce.h)
//             with ReduceArgs::ss = sd, every product rounded in its order (ss first, then w); mean passes sd = 1/count
//   WINNERS   adjoint of max / min over copy_xj: c[j][f] = Σ_p (x[j][f] == y[col_p][f] ? dy[col_p][f] : 0) — maxmin_grad_range
//             (maxmin_grad.h, the loop of maxmin_grad_kernel); every tie receives Δ, as in NNlib
//   IDENTITY  c[j] = dy[j]: a layer's root term, or a type that is its own source
//   MASKED    c[j][f] = (y[j][f] == out[j][f]) ? dy[j][f] : 0: the pullback of one term of foldl(max | min, ...); every tying term receives Δ
//             (this project's own rule — see include/gnnmp.h)
// A row longer than its plan's split threshold is walked whole by its lane group (correct, slow for hubs: gnnmp/backward_hetero.py sends
// such graphs to the composition).  Nothing here touches a plan's workspace: the tables travel by value in the kernel arguments, the
// export neither allocates nor synchronises.
#include "csr_reduce.h"
#include "maxmin_grad.h"

namespace gnnmp {

enum { HG_LINEAR = 0, HG_WINNERS = 1, HG_IDENTITY = 2, HG_MASKED = 3 };

struct HeteroGradRel {
    const uint32_t *rowptr;     // transposed plan; null: identity / masked identity
    const int32_t *col, *eid;
    const float *dy;            // [n_dst][D]; identity: [n_src][D]
    const float *w;             // [n_edges] original order, nullable
    const float *sd;            // [n_dst] per gathered row, nullable
    const float *y;             // winners: [n_dst][D]; masked: [n_src][D]
    const float *out;           // masked: [n_src][D]
    uint32_t n_edges;
    int mode;
};
struct HeteroGradSrc {
    float *dx;                  // [n_src][D]
    const float *x;             // [n_src][D], read when load_x
    int n_src;
    int load_x;                 // some relation of this type is HG_WINNERS
    int rel_beg, rel_end;       // its relations in HeteroGradArgs::rel, in sum order
    uint32_t blk_end;           // one past its last block (prefix of block counts)
};
struct HeteroGradArgs {
    HeteroGradSrc src[GNNMP_HETERO_MAX_REL];
    HeteroGradRel rel[GNNMP_HETERO_MAX_REL];
    int n_srcs, D, log2g, waves;
};
static_assert(sizeof(HeteroGradArgs) < 4096, "the tables travel by value in the kernel arguments");

// SCALED: some relation of the call carries w or sd (a relation without one multiplies by 1.0f: the same bits)
template <int VEC, bool SCALED>
__global__ void __launch_bounds__(256) hetero_grad_rows_kernel(const HeteroGradArgs h) {
    int s = 0;
    uint32_t b0 = 0;
    while (s < h.n_srcs - 1 && blockIdx.x >= h.src[s].blk_end) b0 = h.src[s++].blk_end;
    const HeteroGradSrc &ss = h.src[s];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int G = 1 << h.log2g;
    const int lig = lane & (G - 1), gbase = lane - lig;
    const int64_t row64 = ((int64_t)(blockIdx.x - b0) * h.waves + wave) * (64 >> h.log2g) + (lane >> h.log2g);
    if (row64 >= ss.n_src) return;
    const int row = (int)row64;
    const int f0 = ((int)blockIdx.y * G + lig) * VEC;
    const bool active = f0 < h.D;
    const int64_t at = (int64_t)row * h.D + f0;
    float run[VEC], xv[VEC];
#pragma unroll
    for (int q = 0; q < VEC; ++q) run[q] = xv[q] = 0.0f;
    if (ss.load_x && active) Vec<VEC>::load(ss.x + at, xv);
    for (int k = ss.rel_beg; k < ss.rel_end; ++k) {
        const HeteroGradRel &r = h.rel[k];
        float acc[VEC];
#pragma unroll
        for (int q = 0; q < VEC; ++q) acc[q] = 0.0f;
        switch (r.mode) {
            case HG_LINEAR: {
                ReduceArgs a = {};
                a.rows.col = r.col;
                a.rows.eid = r.eid;
                a.rows.n_edges = r.n_edges;
                a.x = r.dy;
                a.w = r.w;
                a.ss = r.sd;
                a.D = h.D;
                reduce_range<VEC, OP_SUM, SCALED, 8>(a, r.rowptr[row], r.rowptr[row + 1], lig, gbase, G, f0, active, acc);
                break;
            }
            case HG_WINNERS:
                maxmin_grad_range<VEC, 4>(r.col, r.y, r.dy, h.D, r.rowptr[row], r.rowptr[row + 1], lig, gbase, G, f0, active, xv, acc);
                break;
            case HG_IDENTITY:
                if (active) Vec<VEC>::load(r.dy + at, acc);
                break;
            default: {
                float yv[VEC], ov[VEC];
#pragma unroll
                for (int q = 0; q < VEC; ++q) yv[q] = ov[q] = 0.0f;
                if (active) {
                    Vec<VEC>::load(r.dy + at, acc);
                    Vec<VEC>::load(r.y + at, yv);
                    Vec<VEC>::load(r.out + at, ov);
                }
#pragma unroll
                for (int q = 0; q < VEC; ++q) acc[q] = yv[q] == ov[q] ? acc[q] : 0.0f;
                break;
            }
        }
#pragma unroll
        for (int q = 0; q < VEC; ++q) run[q] = k == ss.rel_beg ? acc[q] : run[q] + acc[q];
    }
    if (active) Vec<VEC>::store(ss.dx + at, run);
}

}  // namespace gnnmp

using namespace gnnmp;

extern "C" int gnnmp_hetero_propagate_grad_f32(const gnnmp_hetero_src_t *srcs, int n_srcs, int64_t D, gnnmp_stream_t stream) {
    if (!srcs || n_srcs < 1) return fail(GNNMP_EINVAL, "hetero_propagate_grad: null or empty source table");
    if (D < 1 || D > (1 << 20)) return fail(GNNMP_EINVAL, "hetero_propagate_grad: bad D %lld", (long long)D);
    int64_t n_rel = 0;
    for (int s = 0; s < n_srcs; ++s) {
        if (srcs[s].n_rel < 1 || !srcs[s].rels) return fail(GNNMP_EINVAL, "hetero_propagate_grad: source %d has no relation table", s);
        n_rel += srcs[s].n_rel;
    }
    if (n_rel > GNNMP_HETERO_MAX_REL)
        return fail(GNNMP_EUNSUPPORTED, "hetero_propagate_grad: %lld relations in one call (at most %d)", (long long)n_rel, GNNMP_HETERO_MAX_REL);
    HeteroGradArgs h = {};
    h.n_srcs = n_srcs;
    h.D = (int)D;
    uintptr_t align = 0;
    bool scaled = false;
    int k = 0;
    for (int s = 0; s < n_srcs; ++s) {
        const gnnmp_hetero_src_t &t = srcs[s];
        if (t.n_src < 0 || t.n_src >= INT32_MAX) return fail(GNNMP_EINVAL, "hetero_propagate_grad: source %d: bad n_src %lld", s, (long long)t.n_src);
        if (!t.dx && t.n_src > 0) return fail(GNNMP_EINVAL, "hetero_propagate_grad: source %d: null dx", s);
        HeteroGradSrc &o = h.src[s];
        o.dx = t.dx;
        o.x = t.x;
        o.n_src = (int)t.n_src;
        o.rel_beg = k;
        align |= reinterpret_cast<uintptr_t>(t.dx);
        for (int j = 0; j < t.n_rel; ++j, ++k) {
            const gnnmp_hetero_rel_grad_t &r = t.rels[j];
            HeteroGradRel &q = h.rel[k];
            const gnnmp_graph_t *p = r.plan_t;
            if (r.out && !r.y) return fail(GNNMP_EINVAL, "hetero_propagate_grad: source %d relation %d: out without y", s, j);
            if (p && r.out) return fail(GNNMP_EINVAL, "hetero_propagate_grad: source %d relation %d: out belongs to identity relations", s, j);
            if (!p && r.y && !r.out) return fail(GNNMP_EINVAL, "hetero_propagate_grad: source %d relation %d: an identity relation with y needs out", s, j);
            if (p && r.y && (r.w || r.sd))
                return fail(GNNMP_EINVAL, "hetero_propagate_grad: source %d relation %d: y (max / min) together with w or sd", s, j);
            if (p && p->n_dst != t.n_src)
                return fail(GNNMP_EINVAL, "hetero_propagate_grad: source %d relation %d: the transposed plan has %lld rows, the table %lld sources", s, j,
                            (long long)p->n_dst, (long long)t.n_src);
            const bool reads = t.n_src > 0 && (!p || p->n_total > 0);
            if (!r.dy && reads) return fail(GNNMP_EINVAL, "hetero_propagate_grad: source %d relation %d: null dy", s, j);
            if (p && r.y && !t.x && reads) return fail(GNNMP_EINVAL, "hetero_propagate_grad: source %d relation %d: null x (max / min)", s, j);
            q.dy = r.dy;
            align |= reinterpret_cast<uintptr_t>(r.dy);
            if (p) {
                q.rowptr = p->rowptr;
                q.col = p->col;
                q.eid = p->eid;
                q.n_edges = (uint32_t)p->n_edges;
                if (r.y) {
                    q.mode = HG_WINNERS;
                    q.y = r.y;
                    if (t.x) o.load_x = 1;      // (null only where no slot exists to compare against)
                    align |= reinterpret_cast<uintptr_t>(r.y) | reinterpret_cast<uintptr_t>(t.x);
                } else {
                    q.mode = HG_LINEAR;
                    q.w = r.w;
                    q.sd = r.sd;
                    scaled = scaled || r.w || r.sd;
                }
            } else if (r.out) {
                q.mode = HG_MASKED;
                q.y = r.y;
                q.out = r.out;
                align |= reinterpret_cast<uintptr_t>(r.y) | reinterpret_cast<uintptr_t>(r.out);
            } else {
                q.mode = HG_IDENTITY;
            }
        }
        o.rel_end = k;
    }
    const int vec = pick_vec(D, reinterpret_cast<const void *>(align), nullptr);
    h.log2g = pick_log2g((D + vec - 1) / vec);
    h.waves = 4;
    const int rows_per_block = (64 >> h.log2g) * h.waves;
    int64_t blocks = 0;
    for (int s = 0; s < n_srcs; ++s) {
        blocks += (srcs[s].n_src + rows_per_block - 1) / rows_per_block;
        if (blocks >= INT32_MAX) return fail(GNNMP_EUNSUPPORTED, "hetero_propagate_grad: too many row blocks");
        h.src[s].blk_end = (uint32_t)blocks;
    }
    if (blocks == 0) return GNNMP_OK;
    const dim3 grid((unsigned)blocks, (unsigned)feature_tiles(D, vec, h.log2g));
    with_vec(vec, [&](auto V) {
        constexpr int VEC = decltype(V)::value;
        if (scaled)
            hetero_grad_rows_kernel<VEC, true><<<grid, 64 * h.waves, 0, (hipStream_t)stream>>>(h);
        else
            hetero_grad_rows_kernel<VEC, false><<<grid, 64 * h.waves, 0, (hipStream_t)stream>>>(h);
    });
    GNNMP_LAUNCH_CHECK("hetero_grad_rows_kernel");
    return GNNMP_OK;
}
