// attn_edge.hip — neighbourhood attention with a per-edge feature ROW, forward and pullback: gatv2_conv and transformer_conv with `e`
// (GNNlib/src/layers/conv.jl:171-214 and :553-629).  F = dense_e(e) | W6(e), [n_edges][H*C] in ORIGINAL edge order; k = the original
// position of edge j -> i, fetched through the plan's eid like gat_fused.hip's per-edge score.  Per head:
//   GATV2  z_c = Q_ic + K_jc + F_kc,  l_ij = Σ_c a_c lrelu(z_c),        o_i = Σ_j α_ij K_j              (the value carries no F)
//   DOT    l_ij = Q_i . (K_j + F_k) / scale,                             o_i = Σ_j α_ij (V_j + F_k)
// The forward is gat_fused.hip's online softmax (running max and denominator, one rescale per batch of U edges, head sums by
// group_sum) with U further loads of F_k per batch.  The pullback is attn_backward.hip's two passes:
//   g_ij = Δ_i . val_ij,   D_i = Σ_j α_ij g_ij,   dl_ij = α_ij (g_ij - D_i),   α rebuilt from the forward's (m_i, den_i)
//   pass 1 (plan):    D_i, dQ_i (GATV2: the per-destination terms of da), the line (m, 1/den, D) per (i, h)
//   pass 2 (plan_t):  per source j, every out-edge once: dK_j, dV_j, and dF_k — ONE plain vector store at the slot's eid
//     GATV2  dF_kc = a_c dl_ij s_c (s = lrelu'(z))                       DOT  dF_k = dl_ij Q_i / scale + α_ij Δ_i
// Both passes are whole-row walks (slotwalk.h): the plans are only read, there is no scratch and no atomic, every output element is
// written exactly once, two calls give equal bits and a capture needs no eager call first.  The price, as in the other training
// kernels of that kit: a hub row is walked by ONE lane group.
//
// U = 4 edges a batch everywhere, chosen from what hipcc reports (VEC = 4, four lanes a head; GATV2 / DOT; no instance uses scratch), NOT
// from a measurement — a slot keeps K_j and F_k live (DOT: V_j too), twice the e-less kernel's registers per slot:
//              forward                 pass 1                  pass 2
//   U = 2      59 / 62 VGPRs, 8 waves   81 / 74, 5 / 6 waves    82 / 79, 5 / 6 waves
//   U = 4      68 / 72, 7 waves         109 / 102, 4 waves      94 / 116, 5 / 4 waves
//   U = 8      108 / 105, 4 waves       133 / 135, 3 waves      153 / 180, 3 / 2 waves
// Row loads in flight per SIMD = (2 | 3) U x waves: the forward has 56 / 84 at U = 4 against 32 / 48 at U = 2; U = 8 has a few more
// (64 / 96) but only 4 waves to hide the head butterflies and exponentials behind.  The pullback passes have 32 .. 48 at U = 4, 20 .. 36
// at U = 2 and as many or fewer at U = 8, and U = 4 is the e-less pullback's U.  The run-time-lane-count instances
// (LPH = 0: v < 4 or a head that is no power of two) take up to 128 VGPRs in pass 2, still without scratch.
#include "launch.h"
#include "slotwalk.h"

namespace gnnmp {

struct AttnEdgeArgs {
    PlanRows rows;            // of the plan the running pass walks, whole rows
    RowGeom geom;
    const float *Q, *K, *V;   // [n_dst][D], [n_src][D], [n_src][D]
    const float *F;           // [n_edges][D]
    const float *a;           // GATV2: [H][C]
    const float *bias;        // forward: [D] or null
    const float *dout;        // Δ [n_dst][D]
    const float *stats_in;    // pullback: [n_dst][H][2]
    float *out, *stats;       // forward
    float *line;              // [n_dst][H][4] = (m, 1/den, D, 0)
    float *dQ, *dA;           // [n_dst][D]
    float *dK, *dV;           // [n_src][D]  (GATV2: dK holds the whole gradient of K)
    float *dF;                // [n_edges][D]
    int H, C, D, lph, act;
    float slope, scale;
};

constexpr int EDGE_U = 4;

__device__ __forceinline__ float lrelu_e(float x, float slope) { return x > 0.0f ? x : x * slope; }

// what a lane keeps for its row: the feature slice it owns (idle lanes shadow lane 0 with zero coefficients: no load needs a predicate)
template <int VEC>
struct EdgeLane {
    int f0, fc, h;
    bool active;
    float ca[VEC];
};
template <int VEC, int MODE>
__device__ __forceinline__ EdgeLane<VEC> edge_lane(const AttnEdgeArgs &a, int lig) {
    EdgeLane<VEC> r;
    r.f0 = lig * VEC;
    r.active = r.f0 < a.D;
    r.fc = r.active ? r.f0 : 0;
    r.h = r.fc / a.C;
#pragma unroll
    for (int q = 0; q < VEC; ++q) r.ca[q] = 0.0f;
    if (MODE == GNNMP_ATTN_GATV2 && r.active) {
        const float *ah = a.a + (int64_t)r.h * a.C + (r.fc - r.h * a.C);
#pragma unroll
        for (int q = 0; q < VEC; ++q) r.ca[q] = ah[q];
    }
    return r;
}
template <int VEC>
__device__ __forceinline__ void load_masked(const float *p, bool active, float v[VEC]) {
    Vec<VEC>::load(p, v);
#pragma unroll
    for (int q = 0; q < VEC; ++q) v[q] = active ? v[q] : 0.0f;
}

// ---- forward ------------------------------------------------------------------------------------------------------------------------
template <int VEC, int U, int LPH, int MODE>
__global__ void __launch_bounds__(256) attn_edge_fwd_kernel(const AttnEdgeArgs a) {
    VRow vr;
    if (!decode_vrow<VROW_WHOLE>(a.rows, a.geom, blockIdx.x, vr)) return;
    const EdgeLane<VEC> r = edge_lane<VEC, MODE>(a, vr.lig);
    float qi[VEC];
    load_masked<VEC>(a.Q + (int64_t)vr.row * a.D + r.fc, r.active, qi);
    float m = -__builtin_inff(), den = 0.0f, acc[VEC];
#pragma unroll
    for (int q = 0; q < VEC; ++q) acc[q] = 0.0f;
    for (uint32_t base = vr.beg; base < vr.end; base += vr.G) {   // slots are unsigned 32-bit (rowwalk.h)
        const Slots s = load_slots<true, true>(a.rows.col, a.rows.eid, base, vr.end, vr.lig, vr.G);
        for (int j = 0; j < s.n; j += U) {
            int cj[U];
            uint32_t ej[U];
            bcast_slots<U, true, true>(s, vr.gbase, j, cj, ej);
            float kv[U][VEC], fv[U][VEC];
            float vv[MODE == GNNMP_ATTN_DOT ? U : 1][VEC];      // V_j when it is a different array
#pragma unroll
            for (int u = 0; u < U; ++u) {
                Vec<VEC>::load(a.K + (int64_t)cj[u] * a.D + r.fc, kv[u]);
                if (MODE == GNNMP_ATTN_DOT) Vec<VEC>::load(a.V + (int64_t)cj[u] * a.D + r.fc, vv[MODE == GNNMP_ATTN_DOT ? u : 0]);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) Vec<VEC>::load(a.F + (int64_t)ej[u] * a.D + r.fc, fv[u]);
            float l[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                l[u] = 0.0f;
#pragma unroll
                for (int q = 0; q < VEC; ++q) {
                    if (MODE == GNNMP_ATTN_GATV2) l[u] = fmaf(r.ca[q], lrelu_e((qi[q] + kv[u][q]) + fv[u][q], a.slope), l[u]);
                    if (MODE == GNNMP_ATTN_DOT) l[u] = fmaf(qi[q], kv[u][q] + fv[u][q], l[u]);
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) l[u] = group_sum<LPH>(l[u], a.lph);
            float mn = m;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                float lu = l[u];
                if (MODE == GNNMP_ATTN_DOT) lu = lu / a.scale;
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
                for (int q = 0; q < VEC; ++q) {
                    const float val = MODE == GNNMP_ATTN_DOT ? vv[MODE == GNNMP_ATTN_DOT ? u : 0][q] + fv[u][q] : kv[u][q];
                    acc[q] = fmaf(pe, val, acc[q]);
                }
            }
        }
    }
    if (!r.active) return;
    if (vr.end > vr.beg) {
#pragma unroll
        for (int q = 0; q < VEC; ++q) acc[q] = acc[q] / den;
    }
    if (a.stats && (r.f0 % a.C) == 0) {
        float *st = a.stats + ((int64_t)vr.row * a.H + r.h) * 2;
        st[0] = m;
        st[1] = den;
    }
    if (a.bias) {
#pragma unroll
        for (int q = 0; q < VEC; ++q) acc[q] = acc[q] + a.bias[r.f0 + q];
    }
    if (a.act == GNNMP_ACT_RELU) {
#pragma unroll
        for (int q = 0; q < VEC; ++q) acc[q] = acc[q] < 0.0f ? 0.0f : acc[q];
    }
    Vec<VEC>::store(a.out + (int64_t)vr.row * a.D + r.f0, acc);
}

// ---- pullback, pass 1: the destinations ------------------------------------------------------------------------------------------------
template <int VEC, int U, int LPH, int MODE>
__global__ void __launch_bounds__(256) attn_edge_bwd_dst_kernel(const AttnEdgeArgs a) {
    constexpr int NA = MODE == GNNMP_ATTN_GATV2 ? 4 : 2;    // Σαgf and Σαf for f = s_c (+ f = lrelu(z_c) for da) | f = K_jc + F_kc
    VRow vr;
    if (!decode_vrow<VROW_WHOLE>(a.rows, a.geom, blockIdx.x, vr)) return;
    const EdgeLane<VEC> r = edge_lane<VEC, MODE>(a, vr.lig);
    const int row = vr.row;
    float qi[VEC], di[VEC];
    load_masked<VEC>(a.Q + (int64_t)row * a.D + r.fc, r.active, qi);
    load_masked<VEC>(a.dout + (int64_t)row * a.D + r.fc, r.active, di);
    const float m = a.stats_in[((int64_t)row * a.H + r.h) * 2];
    const float rden = 1.0f / a.stats_in[((int64_t)row * a.H + r.h) * 2 + 1];
    float S1 = 0.0f, acc[NA][VEC];
#pragma unroll
    for (int k = 0; k < NA; ++k)
#pragma unroll
        for (int q = 0; q < VEC; ++q) acc[k][q] = 0.0f;
    for (uint32_t base = vr.beg; base < vr.end; base += vr.G) {
        const Slots s = load_slots<true, true>(a.rows.col, a.rows.eid, base, vr.end, vr.lig, vr.G);
        for (int j = 0; j < s.n; j += U) {
            int cj[U];
            uint32_t ej[U];
            bcast_slots<U, true, true>(s, vr.gbase, j, cj, ej);
            float kv[U][VEC], fv[U][VEC];
            float vv[MODE == GNNMP_ATTN_DOT ? U : 1][VEC];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                Vec<VEC>::load(a.K + (int64_t)cj[u] * a.D + r.fc, kv[u]);
                if (MODE == GNNMP_ATTN_DOT) Vec<VEC>::load(a.V + (int64_t)cj[u] * a.D + r.fc, vv[MODE == GNNMP_ATTN_DOT ? u : 0]);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) Vec<VEC>::load(a.F + (int64_t)ej[u] * a.D + r.fc, fv[u]);
            float l[U], g[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                l[u] = 0.0f;
                g[u] = 0.0f;
#pragma unroll
                for (int q = 0; q < VEC; ++q) {
                    if (MODE == GNNMP_ATTN_GATV2) {
                        g[u] = fmaf(di[q], kv[u][q], g[u]);
                        kv[u][q] = (qi[q] + kv[u][q]) + fv[u][q];      // from here on: z_c
                        l[u] = fmaf(r.ca[q], lrelu_e(kv[u][q], a.slope), l[u]);
                    }
                    if (MODE == GNNMP_ATTN_DOT) {
                        g[u] = fmaf(di[q], vv[MODE == GNNMP_ATTN_DOT ? u : 0][q] + fv[u][q], g[u]);
                        kv[u][q] = kv[u][q] + fv[u][q];                // from here on: K_j + F_k
                        l[u] = fmaf(qi[q], kv[u][q], l[u]);
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                l[u] = group_sum<LPH>(l[u], a.lph);
                g[u] = group_sum<LPH>(g[u], a.lph);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                float lu = l[u];
                if (MODE == GNNMP_ATTN_DOT) lu = lu / a.scale;
                float al = expf(lu - m) * rden;
                al = (j + u < s.n) ? al : 0.0f;
                const float ag = al * g[u];
                S1 += ag;
#pragma unroll
                for (int q = 0; q < VEC; ++q) {
                    if (MODE == GNNMP_ATTN_GATV2) {
                        const float z = kv[u][q];
                        const float sl = z > 0.0f ? 1.0f : a.slope;
                        const float lr = lrelu_e(z, a.slope);
                        acc[0][q] = fmaf(ag, sl, acc[0][q]);
                        acc[1][q] = fmaf(al, sl, acc[1][q]);
                        acc[NA - 2][q] = fmaf(ag, lr, acc[NA - 2][q]);
                        acc[NA - 1][q] = fmaf(al, lr, acc[NA - 1][q]);
                    }
                    if (MODE == GNNMP_ATTN_DOT) {
                        acc[0][q] = fmaf(ag, kv[u][q], acc[0][q]);
                        acc[1][q] = fmaf(al, kv[u][q], acc[1][q]);
                    }
                }
            }
        }
    }
    if (!r.active) return;
    float dq[VEC];
#pragma unroll
    for (int q = 0; q < VEC; ++q) {
        if (MODE == GNNMP_ATTN_GATV2) dq[q] = r.ca[q] * (acc[0][q] - S1 * acc[1][q]);
        if (MODE == GNNMP_ATTN_DOT) dq[q] = (acc[0][q] - S1 * acc[1][q]) / a.scale;
    }
    Vec<VEC>::store(a.dQ + (int64_t)row * a.D + r.f0, dq);
    if (MODE == GNNMP_ATTN_GATV2) {
        float da[VEC];
#pragma unroll
        for (int q = 0; q < VEC; ++q) da[q] = acc[NA - 2][q] - S1 * acc[NA - 1][q];
        Vec<VEC>::store(a.dA + (int64_t)row * a.D + r.f0, da);
    }
    if ((r.f0 % a.C) == 0) {
        float *ln = a.line + ((int64_t)row * a.H + r.h) * 4;
        ln[0] = m;
        ln[1] = vr.end > vr.beg ? rden : 0.0f;
        ln[2] = S1;
        ln[3] = 0.0f;
    }
}

// ---- pullback, pass 2: the sources; every edge is one slot of the reversed plan, so dF_k is written once ------------------------------
template <int VEC, int U, int LPH, int MODE>
__global__ void __launch_bounds__(256) attn_edge_bwd_src_kernel(const AttnEdgeArgs a) {
    VRow vr;
    if (!decode_vrow<VROW_WHOLE>(a.rows, a.geom, blockIdx.x, vr)) return;
    const EdgeLane<VEC> r = edge_lane<VEC, MODE>(a, vr.lig);
    const int row = vr.row;
    float kj[VEC], vj[VEC];
    load_masked<VEC>(a.K + (int64_t)row * a.D + r.fc, r.active, kj);
    load_masked<VEC>(a.V + (int64_t)row * a.D + r.fc, r.active, vj);
    float dk[VEC], dv[VEC];
#pragma unroll
    for (int q = 0; q < VEC; ++q) dk[q] = dv[q] = 0.0f;
    for (uint32_t base = vr.beg; base < vr.end; base += vr.G) {
        const Slots s = load_slots<true, true>(a.rows.col, a.rows.eid, base, vr.end, vr.lig, vr.G);
        for (int j = 0; j < s.n; j += U) {
            int ci[U];
            uint32_t ej[U];
            bcast_slots<U, true, true>(s, vr.gbase, j, ci, ej);
            float dd[U][VEC], qq[U][VEC], fv[U][VEC];
            float4 ln[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                Vec<VEC>::load(a.dout + (int64_t)ci[u] * a.D + r.fc, dd[u]);
                Vec<VEC>::load(a.Q + (int64_t)ci[u] * a.D + r.fc, qq[u]);
                ln[u] = *reinterpret_cast<const float4 *>(a.line + ((int64_t)ci[u] * a.H + r.h) * 4);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                // DOT: Δ_i and Q_i are not masked here (K_j and V_j are), so F_k of an idle lane must not meet them in g and l
                if (MODE == GNNMP_ATTN_DOT) load_masked<VEC>(a.F + (int64_t)ej[u] * a.D + r.fc, r.active, fv[u]);
                else Vec<VEC>::load(a.F + (int64_t)ej[u] * a.D + r.fc, fv[u]);
            }
            float l[U], g[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                l[u] = 0.0f;
                g[u] = 0.0f;
#pragma unroll
                for (int q = 0; q < VEC; ++q) {
                    if (MODE == GNNMP_ATTN_GATV2) {
                        g[u] = fmaf(dd[u][q], vj[q], g[u]);
                        fv[u][q] = (qq[u][q] + kj[q]) + fv[u][q];      // from here on: z_c, in the forward's order of additions
                        l[u] = fmaf(r.ca[q], lrelu_e(fv[u][q], a.slope), l[u]);
                    }
                    if (MODE == GNNMP_ATTN_DOT) {
                        g[u] = fmaf(dd[u][q], vj[q] + fv[u][q], g[u]);
                        l[u] = fmaf(qq[u][q], kj[q] + fv[u][q], l[u]);
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                l[u] = group_sum<LPH>(l[u], a.lph);
                g[u] = group_sum<LPH>(g[u], a.lph);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                float lu = l[u];
                if (MODE == GNNMP_ATTN_DOT) lu = lu / a.scale;
                float al = expf(lu - ln[u].x) * ln[u].y;
                al = (j + u < s.n) ? al : 0.0f;
                const float dl = al * (g[u] - ln[u].z);
                float df[VEC];
#pragma unroll
                for (int q = 0; q < VEC; ++q) {
                    dv[q] = fmaf(al, dd[u][q], dv[q]);
                    if (MODE == GNNMP_ATTN_GATV2) {
                        const float sl = fv[u][q] > 0.0f ? 1.0f : a.slope;
                        df[q] = (dl * sl) * r.ca[q];
                        dk[q] = dk[q] + df[q];
                    }
                    if (MODE == GNNMP_ATTN_DOT) {
                        dk[q] = fmaf(dl, qq[u][q], dk[q]);
                        df[q] = fmaf(al, dd[u][q], dl * qq[u][q] / a.scale);
                    }
                }
                // the slots past the batch's end repeat its last edge with α = 0: they own no row of dF
                if (r.active && j + u < s.n) Vec<VEC>::store(a.dF + (int64_t)ej[u] * a.D + r.f0, df);
            }
        }
    }
    if (!r.active) return;
    if (MODE == GNNMP_ATTN_GATV2) {
#pragma unroll
        for (int q = 0; q < VEC; ++q) dk[q] = dk[q] + dv[q];    // V is K: one gradient
        Vec<VEC>::store(a.dK + (int64_t)row * a.D + r.f0, dk);
    } else {
#pragma unroll
        for (int q = 0; q < VEC; ++q) dk[q] = dk[q] / a.scale;
        Vec<VEC>::store(a.dK + (int64_t)row * a.D + r.f0, dk);
        Vec<VEC>::store(a.dV + (int64_t)row * a.D + r.f0, dv);
    }
}

// da[d] = Σ_i dA[i][d]: one block a column, thread k adds rows k, k + 256, ... in order, then a fixed tree — no scratch, equal bits
__global__ void __launch_bounds__(256) attn_edge_da_kernel(const float *dA, float *da, int64_t N, int D) {
    __shared__ float red[256];
    const int d = blockIdx.x;
    float s = 0.0f;
    for (int64_t i = threadIdx.x; i < N; i += 256) s += dA[i * D + d];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) da[d] = red[0];
}

// f(int_c<VEC>, int_c<LPH>) for the head geometry (DPP butterflies up to 16 lanes a head, as attn_backward.hip)
template <class F>
static void with_head(const HeadGeom &hg, F &&f) {
    with_vec(hg.vec, [&](auto V) { with_lph<decltype(V)::value, 16>(hg.lph, [&](auto L) { f(V, L); }); });
}

}  // namespace gnnmp

using namespace gnnmp;

// The widest v every [.][H*C] array of a call admits — 4 needs 16-byte, 2 needs 8-byte alignment of ALL of them (a null one admits any) —
// narrowed to the head width: gnnmp.h's rule at gnnmp_gat_conv_stats_f32, word for word
static HeadGeom edge_head_geom(int64_t H, int64_t C, std::initializer_list<const float *> arrays) {
    uintptr_t align = 0;
    for (const float *p : arrays) align |= reinterpret_cast<uintptr_t>(p);
    return head_geom(H, C, pick_vec(H * C, reinterpret_cast<const void *>(align), nullptr));
}

// what both exports check of (plan, mode, H, C) before anything else
static int attn_edge_check(const char *who, const gnnmp_graph_t *plan, const void *job, int mode, int64_t H, int64_t C) {
    if (!plan) return fail(GNNMP_EINVAL, "%s: null plan", who);
    if (!job) return fail(GNNMP_EINVAL, "%s: null job", who);
    if (mode != GNNMP_ATTN_GATV2 && mode != GNNMP_ATTN_DOT)
        return fail(GNNMP_EINVAL, "%s: mode %d (edge feature rows enter the GATV2 and DOT logits only)", who, mode);
    if (H <= 0 || C <= 0 || H > (1 << 20) || C > (1 << 20) || H * C > (1 << 20)) return fail(GNNMP_EINVAL, "%s: bad H/C", who);
    return GNNMP_OK;
}

extern "C" int gnnmp_attn_conv_edge_f32(const gnnmp_graph_t *plan, int mode, const gnnmp_attn_edge_t *job, int64_t H, int64_t C,
                                        gnnmp_stream_t stream) {
    const char *who = "attn_conv_edge";
    GNNMP_TRY(attn_edge_check(who, plan, job, mode, H, C));
    if (job->act != GNNMP_ACT_IDENTITY && job->act != GNNMP_ACT_RELU) return fail(GNNMP_EINVAL, "%s: bad act %d", who, job->act);
    GNNMP_TRY(check_edge_plan(who, plan, nullptr, false,
                              "edge features and add_self_loops cannot be combined (GNNlib/src/layers/conv.jl:178-181)"));
    if (plan->n_edges > 0 && !job->F) return fail(GNNMP_EINVAL, "%s: null F", who);
    if (plan->n_dst == 0) return GNNMP_OK;
    const float *Q = job->Q ? job->Q : job->K, *V = job->V ? job->V : job->K;
    if (mode != GNNMP_ATTN_DOT && V != job->K) return fail(GNNMP_EINVAL, "%s: a separate value array needs mode DOT", who);
    if (!job->out || !Q || (mode == GNNMP_ATTN_GATV2 && !job->a) || (plan->n_total > 0 && !job->K))
        return fail(GNNMP_EINVAL, "%s: null pointer", who);
    if (Q == job->K && plan->n_src != plan->n_dst) return fail(GNNMP_EINVAL, "%s: bipartite plan needs a separate Q", who);
    const int D = (int)(H * C);
    const HeadGeom hg = edge_head_geom(H, C, {Q, job->K, V, job->F, job->out});
    if (!hg.fits_wave)
        return fail(GNNMP_EUNSUPPORTED, "%s: the feature row must fit one wave (H*C = %lld, %d lanes > 64)", who, (long long)(H * C), hg.lanes);
    AttnEdgeArgs g = {};
    g.rows = plan_rows_whole(plan);
    g.geom = RowGeom{hg.log2g, 4, 0, 0};
    g.Q = Q;
    g.K = job->K;
    g.V = V;
    g.F = job->F;
    g.a = job->a;
    g.bias = job->bias;
    g.out = job->out;
    g.stats = job->stats;
    g.H = (int)H;
    g.C = (int)C;
    g.D = D;
    g.lph = hg.lph_code;
    g.act = job->act;
    g.slope = job->negative_slope;
    g.scale = job->scale;
    dim3 grid;
    GNNMP_TRY(row_walk_grid(who, g.rows, g.geom, 1, grid));
    with_head(hg, [&](auto V_, auto L) {
        constexpr int VEC = decltype(V_)::value, LPH = decltype(L)::value;
        if (mode == GNNMP_ATTN_GATV2)
            attn_edge_fwd_kernel<VEC, EDGE_U, LPH, GNNMP_ATTN_GATV2><<<grid, 256, 0, (hipStream_t)stream>>>(g);
        else
            attn_edge_fwd_kernel<VEC, EDGE_U, LPH, GNNMP_ATTN_DOT><<<grid, 256, 0, (hipStream_t)stream>>>(g);
    });
    GNNMP_LAUNCH_CHECK("attn_edge_fwd_kernel");
    return GNNMP_OK;
}

extern "C" int gnnmp_attn_conv_edge_grad_f32(const gnnmp_graph_t *plan, const gnnmp_graph_t *plan_t, int mode,
                                             const gnnmp_attn_edge_grad_t *job, int64_t H, int64_t C, gnnmp_stream_t stream) {
    const char *who = "attn_conv_edge_grad";
    GNNMP_TRY(attn_edge_check(who, plan, job, mode, H, C));
    if (!plan_t) return fail(GNNMP_EINVAL, "%s: null plan_t", who);
    GNNMP_TRY(check_edge_plan(who, plan, nullptr, false,
                              "edge features and add_self_loops cannot be combined (GNNlib/src/layers/conv.jl:178-181)"));
    GNNMP_TRY(check_transposed(who, plan, plan_t));
    if (plan->n_edges > 0 && (!job->F || !job->dF)) return fail(GNNMP_EINVAL, "%s: null F / dF", who);
    if (plan->n_dst == 0 && plan->n_src == 0) return GNNMP_OK;
    const float *Q = job->Q ? job->Q : job->K, *V = job->V ? job->V : job->K;
    const bool v2 = mode == GNNMP_ATTN_GATV2;
    if (v2 && V != job->K) return fail(GNNMP_EINVAL, "%s: GATV2 has V = K", who);
    if (!Q || !job->K || !job->stats || !job->dout || !job->line || !job->dQ || !job->dK || (!v2 && !job->dV) || (v2 && (!job->a || !job->dA)))
        return fail(GNNMP_EINVAL, "%s: null pointer", who);
    if ((reinterpret_cast<uintptr_t>(job->line) & 15) != 0) return fail(GNNMP_EINVAL, "%s: line must be 16-byte aligned", who);
    const int D = (int)(H * C);
    const HeadGeom hg = edge_head_geom(H, C, {Q, job->K, V, job->F, job->dout, job->dQ, job->dK, job->dV, job->dA, job->dF});
    if (!hg.fits_wave)
        return fail(GNNMP_EUNSUPPORTED, "%s: the feature row must fit one wave (H*C = %lld, %d lanes > 64)", who, (long long)(H * C), hg.lanes);
    AttnEdgeArgs g = {};
    g.geom = RowGeom{hg.log2g, 4, 0, 0};
    g.Q = Q;
    g.K = job->K;
    g.V = V;
    g.F = job->F;
    g.a = job->a;
    g.dout = job->dout;
    g.stats_in = job->stats;
    g.line = job->line;
    g.dQ = job->dQ;
    g.dA = job->dA;
    g.dK = job->dK;
    g.dV = job->dV;
    g.dF = job->dF;
    g.H = (int)H;
    g.C = (int)C;
    g.D = D;
    g.lph = hg.lph_code;
    g.slope = job->negative_slope;
    g.scale = job->scale;
    dim3 grid;
    g.rows = plan_rows_whole(plan);
    GNNMP_TRY(row_walk_grid(who, g.rows, g.geom, 1, grid));
    if (grid.x > 0) {
        with_head(hg, [&](auto V_, auto L) {
            constexpr int VEC = decltype(V_)::value, LPH = decltype(L)::value;
            if (v2)
                attn_edge_bwd_dst_kernel<VEC, EDGE_U, LPH, GNNMP_ATTN_GATV2><<<grid, 256, 0, (hipStream_t)stream>>>(g);
            else
                attn_edge_bwd_dst_kernel<VEC, EDGE_U, LPH, GNNMP_ATTN_DOT><<<grid, 256, 0, (hipStream_t)stream>>>(g);
        });
        GNNMP_LAUNCH_CHECK("attn_edge_bwd_dst_kernel");
    }
    g.rows = plan_rows_whole(plan_t);
    GNNMP_TRY(row_walk_grid(who, g.rows, g.geom, 1, grid));
    if (grid.x > 0) {
        with_head(hg, [&](auto V_, auto L) {
            constexpr int VEC = decltype(V_)::value, LPH = decltype(L)::value;
            if (v2)
                attn_edge_bwd_src_kernel<VEC, EDGE_U, LPH, GNNMP_ATTN_GATV2><<<grid, 256, 0, (hipStream_t)stream>>>(g);
            else
                attn_edge_bwd_src_kernel<VEC, EDGE_U, LPH, GNNMP_ATTN_DOT><<<grid, 256, 0, (hipStream_t)stream>>>(g);
        });
        GNNMP_LAUNCH_CHECK("attn_edge_bwd_src_kernel");
    }
    if (v2 && job->da) {
        if (plan->n_dst > 0) {
            attn_edge_da_kernel<<<(unsigned)D, 256, 0, (hipStream_t)stream>>>(job->dA, job->da, plan->n_dst, D);
        } else {
            GNNMP_HIP(hipMemsetAsync(job->da, 0, sizeof(float) * (size_t)D, (hipStream_t)stream));
        }
        GNNMP_LAUNCH_CHECK("attn_edge_da_kernel");
    }
    return GNNMP_OK;
}
