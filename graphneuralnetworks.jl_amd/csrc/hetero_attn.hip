// hetero_attn.hip — the attention members of a heterogeneous layer in ONE launch: a destination row is finished over ALL of its incoming
// attention relations before it is stored.  HeteroGraphConv (GraphNeuralNetworks/src/layers/heteroconv.jl:57-86) runs one layer per
// relation and folds the outputs per destination type; with GATConv / GATv2Conv members (gat_conv and gatv2_conv on a relation through
// expand_srcdst, GNNlib/src/layers/conv.jl:112-214) that is R attention launches, R [n_dst][H*C] outputs written and R - 1 passes to
// fold them.  Here, with hetero.hip's decode and attn_edge.hip's walk:
//   - one GROUP of G = 2^k lanes owns one destination row of one destination type and holds its whole [H*C] slice, VEC floats a lane
//     (headgeom.h); blocks [blk_end[d-1], blk_end[d]) belong to type d, so the per-relation mode switch is uniform per block;
//   - per relation the group walks the row WHOLE (slotwalk.h) with the online softmax of gat_fused.hip: running maximum and
//     denominator, one rescale per batch of U edges, head sums by group_sum<LPH>.  The GAT target half a[h][0:C] . Q_i[h] is formed once
//     per row and relation; the source half comes from the K_j row the weighted sum fetches anyway;
//   - it finishes term_r = act_r(o_r + bias_r) in registers, writes stats_r = (m, den) if asked, folds the term into the running value in
//     table order (the first term is copied) and stores the row once after the last relation.
// A relation without a plan is an IDENTITY relation: row i of K [n_dst][H*C] as it is.  No atomics, no plan-owned scratch, plans are only
// read; the tables travel by value in the kernel arguments; the export neither allocates nor synchronises and a capture needs no eager
// call first; two calls give equal bits.  A row longer than its plan's split threshold is walked whole by ONE lane group: correct, slow
// (gnnmp/hetero.py sends graphs with split rows to the per-relation composition).
//
// U = 4 edges a batch, chosen from what hipcc reports for gfx950 (VGPRs / waves per SIMD of hetero_attn_kernel<VEC, U, LPH>, which carries
// both inlined walks; no instance uses scratch) — a COMPILER figure, NOT a measurement:
//              VEC = 4, LPH = 4        VEC = 4, LPH = 16       VEC = 1, LPH = 0 (run-time lane count)
//   U = 2      64 VGPRs, 8 waves       62, 8 waves             42, 8 waves
//   U = 4      71, 7 waves             71, 7 waves             48, 8 waves
//   U = 8      114, 4 waves            114, 4 waves            60, 8 waves
// A slot keeps one K_j row live (VEC registers) next to its logit, so the walk is lighter than attn_edge.hip's (which also holds F_k).
// Row loads in flight per SIMD = U x waves: 28 at U = 4 against 16 at U = 2; U = 8 has 32 but only 4 waves to hide the head butterflies
// and exponentials behind.  The VEC = 4 run-time-lane-count instance (LPH = 0) takes 71 VGPRs at U = 4, VEC = 2 takes 58.
#include "launch.h"
#include "slotwalk.h"

namespace gnnmp {

struct HAttnRel {               // what the whole-row walk reads of a relation; rowptr == null: identity relation
    const uint32_t *rowptr;
    const int32_t *col;
    const float *Q;             // [n_dst][D]
    const float *K;             // [n_src][D]; identity: [n_dst][D]
    const float *a;             // GAT [H][2C] | GATV2 [H][C]
    const float *bias;          // [D] or null
    float *stats;               // [n_dst][H][2] or null
    float slope;
    int mode, act;
};
struct HAttnDst {
    float *out;                 // [n_dst][D]
    int n_dst;
    int combine;                // OP_SUM | OP_MAX | OP_MIN
    int rel_beg, rel_end;       // its relations in HAttnArgs::rel, in fold order
    uint32_t blk_end;           // one past its last block (prefix of block counts)
};
struct HAttnArgs {
    HAttnDst dst[GNNMP_HETERO_MAX_REL];
    HAttnRel rel[GNNMP_HETERO_MAX_REL];
    int n_dsts, H, C, D, log2g, lph, waves;
};
static_assert(GNNMP_HETERO_MAX_REL == 16 && sizeof(HAttnArgs) < 4096, "the tables travel as kernel arguments: 4 KB at most");

constexpr int HATTN_U = 4;

__device__ __forceinline__ float lrelu_h(float x, float slope) { return x > 0.0f ? x : x * slope; }

// the lane's place in its row: VEC features from f0 on, inside head hd; an idle lane (past the row's width) shadows lane 0 with zero
// coefficients and a zero Q slice: no load needs a predicate, its stores are skipped
struct HLane {
    int row, lig, gbase, G, f0, fc, hd;
    bool active;
};

// acc = term_r[row] = act(o + bias) of one attention relation; writes stats_r[row] when asked
template <int VEC, int U, int LPH, int MODE>
__device__ __forceinline__ void hattn_walk(const HAttnRel &r, const HLane &w, int H, int C, int D, int lph, float acc[VEC]) {
    const uint32_t beg = r.rowptr[w.row], end = r.rowptr[w.row + 1];
    float qi[VEC], ca[VEC];
    Vec<VEC>::load(r.Q + (int64_t)w.row * D + w.fc, qi);
#pragma unroll
    for (int q = 0; q < VEC; ++q) {
        qi[q] = w.active ? qi[q] : 0.0f;
        ca[q] = 0.0f;
    }
    float sd = 0.0f;      // GAT: the target half of the logit, once per row and relation
    if (MODE == GNNMP_ATTN_GATV2) {
        if (w.active) {
#pragma unroll
            for (int q = 0; q < VEC; ++q) ca[q] = r.a[w.fc + q];
        }
    } else {
        const float *ah = r.a + (int64_t)w.hd * 2 * C + (w.fc - w.hd * C);
        float t = 0.0f;
        if (w.active) {
#pragma unroll
            for (int q = 0; q < VEC; ++q) {
                t = fmaf(ah[q], qi[q], t);
                ca[q] = ah[C + q];
            }
        }
        sd = group_sum<LPH>(t, lph);
    }
    float m = -__builtin_inff(), den = 0.0f;
#pragma unroll
    for (int q = 0; q < VEC; ++q) acc[q] = 0.0f;
    for (uint32_t base = beg; base < end; base += w.G) {   // slots are unsigned 32-bit (rowwalk.h)
        const Slots s = load_slots<true, false>(r.col, nullptr, base, end, w.lig, w.G);
        for (int j = 0; j < s.n; j += U) {
            int cj[U];
            uint32_t ej[U];
            bcast_slots<U, true, false>(s, w.gbase, j, cj, ej);
            float kv[U][VEC];
#pragma unroll
            for (int u = 0; u < U; ++u) Vec<VEC>::load(r.K + (int64_t)cj[u] * D + w.fc, kv[u]);
            float l[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                l[u] = 0.0f;
#pragma unroll
                for (int q = 0; q < VEC; ++q) {
                    if (MODE == GNNMP_ATTN_GATV2) l[u] = fmaf(ca[q], lrelu_h(qi[q] + kv[u][q], r.slope), l[u]);
                    else l[u] = fmaf(ca[q], kv[u][q], l[u]);
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) l[u] = group_sum<LPH>(l[u], lph);
            float mn = m;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                float lu = l[u];
                if (MODE == GNNMP_ATTN_GAT) lu = lrelu_h(sd + lu, r.slope);
                l[u] = (j + u < s.n) ? lu : -__builtin_inff();
                mn = fmaxf(mn, l[u]);
            }
            const float sc = softmax_exp(m - mn);   // 1 when the maximum did not move, 0 the first time
            den *= sc;
#pragma unroll
            for (int q = 0; q < VEC; ++q) acc[q] *= sc;
            m = mn;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const float pe = softmax_exp(l[u] - m);
                den += pe;
#pragma unroll
                for (int q = 0; q < VEC; ++q) acc[q] = fmaf(pe, kv[u][q], acc[q]);
            }
        }
    }
    if (!w.active) return;
    if (end > beg) {
#pragma unroll
        for (int q = 0; q < VEC; ++q) acc[q] = acc[q] / den;
    }
    if (r.stats && (w.f0 % C) == 0) {
        float *st = r.stats + ((int64_t)w.row * H + w.hd) * 2;
        st[0] = m;
        st[1] = den;
    }
    if (r.bias) {
#pragma unroll
        for (int q = 0; q < VEC; ++q) acc[q] = acc[q] + r.bias[w.f0 + q];
    }
    if (r.act == GNNMP_ACT_RELU) {
#pragma unroll
        for (int q = 0; q < VEC; ++q) acc[q] = acc[q] < 0.0f ? 0.0f : acc[q];
    }
}

template <int VEC, int OP>
__device__ __forceinline__ void hattn_fold(float run[VEC], const float acc[VEC]) {
#pragma unroll
    for (int q = 0; q < VEC; ++q) run[q] = op_apply<OP>(run[q], acc[q]);
}

template <int VEC, int U, int LPH>
__global__ void __launch_bounds__(256) hetero_attn_kernel(const HAttnArgs h) {
    int d = 0;
    uint32_t b0 = 0;
    while (d < h.n_dsts - 1 && blockIdx.x >= h.dst[d].blk_end) b0 = h.dst[d++].blk_end;
    const HAttnDst &dd = h.dst[d];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    HLane w;
    w.G = 1 << h.log2g;
    w.lig = lane & (w.G - 1);
    w.gbase = lane - w.lig;
    const int64_t row64 = ((int64_t)(blockIdx.x - b0) * h.waves + wave) * (64 >> h.log2g) + (lane >> h.log2g);
    if (row64 >= dd.n_dst) return;
    w.row = (int)row64;
    w.f0 = w.lig * VEC;
    w.active = w.f0 < h.D;
    w.fc = w.active ? w.f0 : 0;
    w.hd = w.fc / h.C;
    float run[VEC];
#pragma unroll
    for (int q = 0; q < VEC; ++q) run[q] = 0.0f;
    for (int k = dd.rel_beg; k < dd.rel_end; ++k) {
        const HAttnRel &r = h.rel[k];
        float acc[VEC];
        if (!r.rowptr) {
            Vec<VEC>::load(r.K + (int64_t)w.row * h.D + w.fc, acc);
        } else if (r.mode == GNNMP_ATTN_GATV2) {
            hattn_walk<VEC, U, LPH, GNNMP_ATTN_GATV2>(r, w, h.H, h.C, h.D, h.lph, acc);
        } else {
            hattn_walk<VEC, U, LPH, GNNMP_ATTN_GAT>(r, w, h.H, h.C, h.D, h.lph, acc);
        }
        if (k == dd.rel_beg) {
#pragma unroll
            for (int q = 0; q < VEC; ++q) run[q] = acc[q];
        } else if (dd.combine == OP_MAX) {
            hattn_fold<VEC, OP_MAX>(run, acc);
        } else if (dd.combine == OP_MIN) {
            hattn_fold<VEC, OP_MIN>(run, acc);
        } else {
            hattn_fold<VEC, OP_SUM>(run, acc);
        }
    }
    if (w.active) Vec<VEC>::store(dd.out + (int64_t)w.row * h.D + w.f0, run);
}

}  // namespace gnnmp

using namespace gnnmp;

extern "C" int gnnmp_hetero_attn_f32(const gnnmp_hetero_attn_dst_t *dsts, int n_dsts, int64_t H, int64_t C, gnnmp_stream_t stream) {
    const char *who = "hetero_attn";
    if (!dsts || n_dsts < 1) return fail(GNNMP_EINVAL, "%s: null or empty destination table", who);
    if (H < 1 || C < 1 || H > (1 << 20) || C > (1 << 20) || H * C > (1 << 20))
        return fail(GNNMP_EINVAL, "%s: bad H/C (%lld, %lld)", who, (long long)H, (long long)C);
    int64_t n_rel = 0;
    for (int d = 0; d < n_dsts; ++d) {
        if (dsts[d].n_rel < 1 || !dsts[d].rels) return fail(GNNMP_EINVAL, "%s: destination %d has no relation table", who, d);
        n_rel += dsts[d].n_rel;
    }
    if (n_rel > GNNMP_HETERO_MAX_REL)
        return fail(GNNMP_EUNSUPPORTED, "%s: %lld relations in one call (at most %d)", who, (long long)n_rel, GNNMP_HETERO_MAX_REL);
    HAttnArgs h = {};
    h.n_dsts = n_dsts;
    h.H = (int)H;
    h.C = (int)C;
    h.D = (int)(H * C);
    uintptr_t align = 0;
    int k = 0;
    for (int d = 0; d < n_dsts; ++d) {
        const gnnmp_hetero_attn_dst_t &s = dsts[d];
        if (s.n_dst < 0 || s.n_dst >= INT32_MAX) return fail(GNNMP_EINVAL, "%s: destination %d: bad n_dst %lld", who, d, (long long)s.n_dst);
        if (s.combine != GNNMP_SUM && s.combine != GNNMP_MAX && s.combine != GNNMP_MIN)
            return fail(GNNMP_EINVAL, "%s: destination %d: bad combine %d (+, max or min)", who, d, s.combine);
        if (!s.out && s.n_dst > 0) return fail(GNNMP_EINVAL, "%s: destination %d: null out", who, d);
        HAttnDst &o = h.dst[d];
        o.out = s.out;
        o.n_dst = (int)s.n_dst;
        o.combine = s.combine == GNNMP_MAX ? OP_MAX : (s.combine == GNNMP_MIN ? OP_MIN : OP_SUM);
        o.rel_beg = k;
        align |= reinterpret_cast<uintptr_t>(s.out);
        for (int j = 0; j < s.n_rel; ++j, ++k) {
            const gnnmp_hetero_attn_rel_t &r = s.rels[j];
            HAttnRel &q = h.rel[k];
            const gnnmp_graph_t *p = r.plan;
            if (r.act != GNNMP_ACT_IDENTITY && r.act != GNNMP_ACT_RELU)
                return fail(GNNMP_EINVAL, "%s: destination %d relation %d: bad act %d (identity or relu)", who, d, j, r.act);
            if (p) {
                if (r.mode != GNNMP_ATTN_GAT && r.mode != GNNMP_ATTN_GATV2)
                    return fail(GNNMP_EINVAL, "%s: destination %d relation %d: bad mode %d (GAT or GATV2)", who, d, j, r.mode);
                if (p->n_dst != s.n_dst)
                    return fail(GNNMP_EINVAL, "%s: destination %d relation %d: the plan has %lld destinations, the table %lld", who, d, j,
                                (long long)p->n_dst, (long long)s.n_dst);
                if (p->self_loops)
                    return fail(GNNMP_EINVAL, "%s: destination %d relation %d: the plan adds self loops of its own (a relation has none)", who, d, j);
                if (s.n_dst > 0 && (!r.Q || !r.a)) return fail(GNNMP_EINVAL, "%s: destination %d relation %d: null Q / a", who, d, j);
                if (s.n_dst > 0 && p->n_total > 0 && !r.K) return fail(GNNMP_EINVAL, "%s: destination %d relation %d: null K", who, d, j);
                q.rowptr = p->rowptr;
                q.col = p->col;
                q.Q = r.Q;
                q.a = r.a;
                q.bias = r.bias;
                q.stats = r.stats;
                q.slope = r.negative_slope;
                q.mode = r.mode;
                q.act = r.act;
                align |= reinterpret_cast<uintptr_t>(r.Q);
            } else if (s.n_dst > 0 && !r.K) {
                return fail(GNNMP_EINVAL, "%s: destination %d relation %d: null K of an identity relation", who, d, j);
            }
            q.K = r.K;
            align |= reinterpret_cast<uintptr_t>(r.K);
        }
        o.rel_end = k;
    }
    const HeadGeom hg = head_geom(H, C, pick_vec(H * C, reinterpret_cast<const void *>(align), nullptr));
    if (!hg.fits_wave)
        return fail(GNNMP_EUNSUPPORTED, "%s: the feature row must fit one wave (H*C = %lld, %d lanes > 64)", who, (long long)(H * C), hg.lanes);
    h.log2g = hg.log2g;
    h.lph = hg.lph_code;
    h.waves = 4;
    const int rows_per_block = (64 >> h.log2g) * h.waves;
    int64_t blocks = 0;
    for (int d = 0; d < n_dsts; ++d) {
        blocks += (dsts[d].n_dst + rows_per_block - 1) / rows_per_block;
        if (blocks >= INT32_MAX) return fail(GNNMP_EUNSUPPORTED, "%s: too many row blocks", who);
        h.dst[d].blk_end = (uint32_t)blocks;
    }
    if (blocks == 0) return GNNMP_OK;
    with_vec(hg.vec, [&](auto V) {
        with_lph<decltype(V)::value, 16>(hg.lph, [&](auto L) {
            constexpr int VEC = decltype(V)::value, LPH = decltype(L)::value;
            hetero_attn_kernel<VEC, HATTN_U, LPH><<<(unsigned)blocks, 64 * h.waves, 0, (hipStream_t)stream>>>(h);
        });
    });
    GNNMP_LAUNCH_CHECK("hetero_attn_kernel");
    return GNNMP_OK;
}
