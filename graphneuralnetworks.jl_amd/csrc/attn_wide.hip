// attn_wide.hip — neighbourhood attention on feature rows WIDER than a wave, forward and pullback: gat_conv, gatv2_conv and
// transformer_conv at heads * out > 256 (8 x 64, 4 x 128, 4 x 256 ...), which every one-pass kernel refuses (headgeom.h: fits_wave).
// Attention is independent per head, so nothing has to cross a wave: a wave takes one (row, HEAD TILE) — hpt = min(H, 64 / lph) whole
// heads of lph = C / vec lanes each (headgeom.h: head_tiles), blockIdx.y the tile, the lane's first feature tile * hpt * C + lig * vec.
// The last tile may hold fewer heads: its spare lanes shadow the tile's first lane with zero coefficients (every load has a valid
// address), store nothing, and still take part in every shuffle — a head's lanes never share a butterfly with them.
//   GAT    l = lrelu(a_d . Q_i + a_s . K_j)   V = K          GATV2  l = a . lrelu(Q_i + K_j)   V = K          DOT  l = Q_i . K_j / scale
// The forward is gat_fused.hip's online softmax (running max and denominator, one rescale per batch of U slots, head sums by
// group_sum: DPP for the power-of-two lane counts, lane by lane for C = 100 or 5), bias and σ in registers, (m, den) stored when asked.
// The pullback is attn_backward.hip's two passes, with g_ij = Δ_i . V_j, D_i = Σ_j α_ij g_ij, dl_ij = α_ij (g_ij - D_i), α rebuilt from (m, den):
//   pass 1 (plan, per destination and tile):   D_i, dQ_i, the per-destination terms of da, the line (m, 1/den, D, a_d . Q_i) per (i, h);
//                                              the rebuilt α are normalised by their own sum, so that an error common to a row cancels
//   pass 2 (plan_t, per source and tile):      every out-edge once: dK_j, DOT: dV_j, GAT: the per-source term of da
//   da                                         one block a column over the per-node terms: rows k, k + 256, ... in order, then a fixed tree
// GAT: dz = dl lrelu'(z), dsd_i = Σ_j dz, dss_j = Σ_i dz; dQ_i = a_d dsd_i, dK_j = Σ_i α Δ_i + a_s dss_j, da = [Σ_i dsd_i Q_i | Σ_j dss_j K_j].
// With Q = K on a square plan pass 2 adds dQ_j, which pass 1 has written by then: dK holds the whole gradient of that one array.
// All three kernels are whole-row walks (slotwalk.h), one wave a (row, tile), four waves a block: the plans are only read, there is no
// scratch and no atomic, every output element is written exactly once, two calls give equal bits and a capture needs no eager call
// first.  The price: a hub row is walked by ONE wave per tile, and a source row of 4 D bytes is gathered by `tiles` different waves —
// `col` is read once a tile, 4 bytes against hpt * C * 4 bytes of features.
//
// U = 4 slots a batch, chosen from what hipcc reports for gfx950, NOT from a measurement.  VGPRs (waves a SIMD) of the VEC = 4 instances
// with sixteen lanes a head (C = 64), GAT / GATV2 / DOT; no instance of any of the three kernels uses scratch at any U:
//              forward                       pass 1                        pass 2
//   U = 2      40 / 52 / 51     (8 / 8 / 8)  52 / 75 / 61     (8 / 6 / 8)  56 / 62 / 67    (8 / 8 / 7)
//   U = 4      52 / 76 / 77     (8 / 6 / 6)  65 / 88 / 84     (7 / 5 / 5)  80 / 62 / 64    (6 / 8 / 8)
//   U = 8      76 / 124 / 104   (6 / 4 / 4)  88 / 117 / 120   (5 / 4 / 4)  112 / 90 / 65   (4 / 5 / 7)
// Row loads in flight per SIMD = (1 | DOT: 2) U x waves in the forward and pass 1, (GAT: 1 | 2) U x waves in pass 2: U = 4 has 24 .. 48
// in the forward against 16 .. 32 at U = 2; U = 8 has 32 .. 64 but four waves to hide the head butterflies and exponentials behind, and
// its pullback falls to four waves too.  U = 4 is also the U of attn_backward.hip and attn_edge.hip.  The other U = 4 instances: one to
// eight lanes a head as the table; 32 and 64 lanes a head (two ds_bpermute stages) up to 84 / 100 / 84; the run-time-lane-count
// instances (LPH = 0: v < 4 or a head that is no power of two) up to 70 / 84 / 96 — five waves at the worst.
#include "launch.h"
#include "slotwalk.h"

namespace gnnmp {

struct AttnWideArgs {
    PlanRows rows;            // of the plan the running pass walks, whole rows
    RowGeom geom;             // one wave a row
    const float *Q, *K, *V;   // [n_dst][D], [n_src][D], [n_src][D]
    const float *a;           // GAT: [H][2C]; GATV2: [H][C]
    const float *bias;        // forward: [D] or null
    const float *dout;        // Δ [n_dst][D]
    const float *stats_in;    // pullback: [n_dst][H][2]
    float *out, *stats;       // forward
    float *line;              // [n_dst][H][4] = (m, 1/den, D, GAT: a_d . Q_i)
    float *dQ;                // [n_dst][D]; pass 2 reads it back when Q is K
    float *dA;                // the terms of da of the walked rows: [n_dst][D] in pass 1, [n_src][D] in pass 2 (GAT)
    float *dK, *dV;           // [n_src][D]
    int H, C, D, lph, hpt, act, fold;
    float slope, scale;
};

constexpr int WIDE_U = 4;

__device__ __forceinline__ float lrelu_w(float x, float slope) { return x > 0.0f ? x : x * slope; }

// what a lane keeps for its (row, tile): the feature slice it owns, its head, its slices of a
template <int VEC>
struct WideLane {
    int f0, fc, h;
    bool active;
    float ca[VEC];   // GAT: a_s; GATV2: a
    float cd[VEC];   // GAT: a_d
};
template <int VEC, int MODE>
__device__ __forceinline__ WideLane<VEC> wide_lane(const AttnWideArgs &a, int lig) {
    WideLane<VEC> r;
    const int h0 = (int)blockIdx.y * a.hpt;
    const int nh = min(a.hpt, a.H - h0);
    r.f0 = h0 * a.C + lig * VEC;
    r.active = lig * VEC < nh * a.C;
    r.fc = r.active ? r.f0 : h0 * a.C;
    r.h = r.fc / a.C;
#pragma unroll
    for (int q = 0; q < VEC; ++q) r.ca[q] = r.cd[q] = 0.0f;
    if (r.active && MODE == GNNMP_ATTN_GAT) {
        const float *ah = a.a + (int64_t)r.h * 2 * a.C + (r.fc - r.h * a.C);
#pragma unroll
        for (int q = 0; q < VEC; ++q) {
            r.cd[q] = ah[q];
            r.ca[q] = ah[a.C + q];
        }
    }
    if (r.active && MODE == GNNMP_ATTN_GATV2) {
        const float *ah = a.a + (int64_t)r.h * a.C + (r.fc - r.h * a.C);
#pragma unroll
        for (int q = 0; q < VEC; ++q) r.ca[q] = ah[q];
    }
    return r;
}
template <int VEC>
__device__ __forceinline__ void load_masked_w(const float *p, bool active, float v[VEC]) {
    Vec<VEC>::load(p, v);
#pragma unroll
    for (int q = 0; q < VEC; ++q) v[q] = active ? v[q] : 0.0f;
}
template <int VEC>
__device__ __forceinline__ float dot_w(const float x[VEC], const float y[VEC]) {
    float s = 0.0f;
#pragma unroll
    for (int q = 0; q < VEC; ++q) s = fmaf(x[q], y[q], s);
    return s;
}

// ---- forward ------------------------------------------------------------------------------------------------------------------------
template <int VEC, int U, int LPH, int MODE>
__global__ void __launch_bounds__(256) attn_wide_fwd_kernel(const AttnWideArgs a) {
    constexpr bool DOT = MODE == GNNMP_ATTN_DOT;
    VRow vr;
    if (!decode_vrow<VROW_WHOLE>(a.rows, a.geom, blockIdx.x, vr)) return;
    const WideLane<VEC> r = wide_lane<VEC, MODE>(a, vr.lig);
    float qi[VEC];
    load_masked_w<VEC>(a.Q + (int64_t)vr.row * a.D + r.fc, r.active, qi);
    float s0 = 0.0f;                                   // GAT: a_d . Q_i
    if (MODE == GNNMP_ATTN_GAT) s0 = group_sum<LPH>(dot_w<VEC>(r.cd, qi), a.lph);
    float m = -__builtin_inff(), den = 0.0f, acc[VEC];
#pragma unroll
    for (int q = 0; q < VEC; ++q) acc[q] = 0.0f;
    for (uint32_t base = vr.beg; base < vr.end; base += vr.G) {   // slots are unsigned 32-bit (rowwalk.h)
        const Slots s = load_slots<true, false>(a.rows.col, a.rows.eid, base, vr.end, vr.lig, vr.G);
        for (int j = 0; j < s.n; j += U) {
            int cj[U];
            uint32_t ej[U];
            bcast_slots<U, true, false>(s, vr.gbase, j, cj, ej);
            float kv[U][VEC];
            float vv[DOT ? U : 1][VEC];                // V_j when it is a different array
#pragma unroll
            for (int u = 0; u < U; ++u) {
                Vec<VEC>::load(a.K + (int64_t)cj[u] * a.D + r.fc, kv[u]);
                if (DOT) Vec<VEC>::load(a.V + (int64_t)cj[u] * a.D + r.fc, vv[DOT ? u : 0]);
            }
            float l[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                l[u] = 0.0f;
#pragma unroll
                for (int q = 0; q < VEC; ++q) {
                    if (MODE == GNNMP_ATTN_GAT) l[u] = fmaf(r.ca[q], kv[u][q], l[u]);
                    if (MODE == GNNMP_ATTN_GATV2) l[u] = fmaf(r.ca[q], lrelu_w(qi[q] + kv[u][q], a.slope), l[u]);
                    if (DOT) l[u] = fmaf(qi[q], kv[u][q], l[u]);
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) l[u] = group_sum<LPH>(l[u], a.lph);
            float mn = m;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                float lu = l[u];
                if (MODE == GNNMP_ATTN_GAT) lu = lrelu_w(s0 + lu, a.slope);
                if (DOT) lu = lu / a.scale;
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
                for (int q = 0; q < VEC; ++q) acc[q] = fmaf(pe, DOT ? vv[DOT ? u : 0][q] : kv[u][q], acc[q]);
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
__global__ void __launch_bounds__(256) attn_wide_bwd_dst_kernel(const AttnWideArgs a) {
    constexpr bool GAT = MODE == GNNMP_ATTN_GAT, V2 = MODE == GNNMP_ATTN_GATV2, DOT = MODE == GNNMP_ATTN_DOT;
    constexpr int NA = V2 ? 4 : 2;    // Σαgf and Σαf for f = s_c (+ f = lrelu(z_c) for da) | f = K_jc; GAT keeps three scalars instead
    VRow vr;
    if (!decode_vrow<VROW_WHOLE>(a.rows, a.geom, blockIdx.x, vr)) return;
    const WideLane<VEC> r = wide_lane<VEC, MODE>(a, vr.lig);
    const int row = vr.row;
    float qi[VEC], di[VEC];
    load_masked_w<VEC>(a.Q + (int64_t)row * a.D + r.fc, r.active, qi);
    load_masked_w<VEC>(a.dout + (int64_t)row * a.D + r.fc, r.active, di);
    float sd = 0.0f;
    if (GAT) sd = group_sum<LPH>(dot_w<VEC>(r.cd, qi), a.lph);
    const float m = a.stats_in[((int64_t)row * a.H + r.h) * 2];
    const float rden = 1.0f / a.stats_in[((int64_t)row * a.H + r.h) * 2 + 1];
    float S0 = 0.0f, S1 = 0.0f, S2 = 0.0f, S3 = 0.0f, acc[NA][VEC];
#pragma unroll
    for (int k = 0; k < NA; ++k)
#pragma unroll
        for (int q = 0; q < VEC; ++q) acc[k][q] = 0.0f;
    for (uint32_t base = vr.beg; base < vr.end; base += vr.G) {
        const Slots s = load_slots<true, false>(a.rows.col, a.rows.eid, base, vr.end, vr.lig, vr.G);
        for (int j = 0; j < s.n; j += U) {
            int cj[U];
            uint32_t ej[U];
            bcast_slots<U, true, false>(s, vr.gbase, j, cj, ej);
            float kv[U][VEC];
            float vv[DOT ? U : 1][VEC];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                Vec<VEC>::load(a.K + (int64_t)cj[u] * a.D + r.fc, kv[u]);
                if (DOT) Vec<VEC>::load(a.V + (int64_t)cj[u] * a.D + r.fc, vv[DOT ? u : 0]);
            }
            float l[U], g[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                l[u] = 0.0f;
                g[u] = 0.0f;
#pragma unroll
                for (int q = 0; q < VEC; ++q) {
                    g[u] = fmaf(di[q], DOT ? vv[DOT ? u : 0][q] : kv[u][q], g[u]);
                    if (GAT) l[u] = fmaf(r.ca[q], kv[u][q], l[u]);
                    if (V2) l[u] = fmaf(r.ca[q], lrelu_w(qi[q] + kv[u][q], a.slope), l[u]);
                    if (DOT) l[u] = fmaf(qi[q], kv[u][q], l[u]);
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
                const float z = sd + lu;                   // GAT
                if (GAT) lu = lrelu_w(z, a.slope);
                if (DOT) lu = lu / a.scale;
                float al = expf(lu - m) * rden;
                al = (j + u < s.n) ? al : 0.0f;
                const float ag = al * g[u];
                S0 += al;
                S1 += ag;
                if (GAT) {
                    const float sl = z > 0.0f ? 1.0f : a.slope;
                    S2 = fmaf(ag, sl, S2);
                    S3 = fmaf(al, sl, S3);
                }
#pragma unroll
                for (int q = 0; q < VEC; ++q) {
                    if (V2) {
                        const float zc = qi[q] + kv[u][q];
                        const float sl = zc > 0.0f ? 1.0f : a.slope;
                        const float lr = lrelu_w(zc, a.slope);
                        acc[0][q] = fmaf(ag, sl, acc[0][q]);
                        acc[1][q] = fmaf(al, sl, acc[1][q]);
                        acc[NA - 2][q] = fmaf(ag, lr, acc[NA - 2][q]);
                        acc[NA - 1][q] = fmaf(al, lr, acc[NA - 1][q]);
                    }
                    if (DOT) {
                        acc[0][q] = fmaf(ag, kv[u][q], acc[0][q]);
                        acc[NA - 1][q] = fmaf(al, kv[u][q], acc[NA - 1][q]);
                    }
                }
            }
        }
    }
    if (!r.active) return;
    // α is rebuilt from a rounded m and re-rounded logits: an error common to the row's edges scales every α alike, and Σ α g f - D Σ α f
    // would turn it into D Σ α f times that error.  Normalised by the α actually summed (S0 = Σ α ≈ 1) the two sums scale together.
    const float rs0 = vr.end > vr.beg ? 1.0f / S0 : 0.0f;
    const float Di = S1 * rs0;
    const float dsd = (S2 - Di * S3) * rs0;                // GAT
    float dq[VEC], da[VEC];
#pragma unroll
    for (int q = 0; q < VEC; ++q) {
        if (GAT) {
            dq[q] = r.cd[q] * dsd;
            da[q] = dsd * qi[q];
        }
        if (V2) {
            dq[q] = r.ca[q] * ((acc[0][q] - Di * acc[1][q]) * rs0);
            da[q] = (acc[NA - 2][q] - Di * acc[NA - 1][q]) * rs0;
        }
        if (DOT) dq[q] = (acc[0][q] - Di * acc[NA - 1][q]) * rs0 / a.scale;
    }
    Vec<VEC>::store(a.dQ + (int64_t)row * a.D + r.f0, dq);
    if (!DOT) Vec<VEC>::store(a.dA + (int64_t)row * a.D + r.f0, da);
    if ((r.f0 % a.C) == 0) {
        float *ln = a.line + ((int64_t)row * a.H + r.h) * 4;
        ln[0] = m;
        ln[1] = vr.end > vr.beg ? rden * rs0 : 0.0f;
        ln[2] = Di;
        ln[3] = sd;
    }
}

// ---- pullback, pass 2: the sources; every edge is one slot of the reversed plan ---------------------------------------------------------
template <int VEC, int U, int LPH, int MODE>
__global__ void __launch_bounds__(256) attn_wide_bwd_src_kernel(const AttnWideArgs a) {
    constexpr bool GAT = MODE == GNNMP_ATTN_GAT, V2 = MODE == GNNMP_ATTN_GATV2, DOT = MODE == GNNMP_ATTN_DOT;
    VRow vr;
    if (!decode_vrow<VROW_WHOLE>(a.rows, a.geom, blockIdx.x, vr)) return;
    const WideLane<VEC> r = wide_lane<VEC, MODE>(a, vr.lig);
    const int row = vr.row;
    float kj[VEC], vj[VEC];
    load_masked_w<VEC>(a.K + (int64_t)row * a.D + r.fc, r.active, kj);
    load_masked_w<VEC>(a.V + (int64_t)row * a.D + r.fc, r.active, vj);
    float ss = 0.0f, dss = 0.0f;                           // GAT: a_s . K_j and Σ_i dz_ij
    if (GAT) ss = group_sum<LPH>(dot_w<VEC>(r.ca, kj), a.lph);
    float dk[VEC], dv[VEC];
#pragma unroll
    for (int q = 0; q < VEC; ++q) dk[q] = dv[q] = 0.0f;
    for (uint32_t base = vr.beg; base < vr.end; base += vr.G) {
        const Slots s = load_slots<true, false>(a.rows.col, a.rows.eid, base, vr.end, vr.lig, vr.G);
        for (int j = 0; j < s.n; j += U) {
            int ci[U];
            uint32_t ej[U];
            bcast_slots<U, true, false>(s, vr.gbase, j, ci, ej);
            float dd[U][VEC];
            float qq[GAT ? 1 : U][VEC];                    // GAT needs no Q_i: the line carries a_d . Q_i
            float4 ln[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                Vec<VEC>::load(a.dout + (int64_t)ci[u] * a.D + r.fc, dd[u]);
                if (!GAT) Vec<VEC>::load(a.Q + (int64_t)ci[u] * a.D + r.fc, qq[GAT ? 0 : u]);
                ln[u] = *reinterpret_cast<const float4 *>(a.line + ((int64_t)ci[u] * a.H + r.h) * 4);
            }
            float l[U], g[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                l[u] = 0.0f;
                g[u] = 0.0f;
#pragma unroll
                for (int q = 0; q < VEC; ++q) {
                    g[u] = fmaf(dd[u][q], vj[q], g[u]);
                    if (V2) l[u] = fmaf(r.ca[q], lrelu_w(qq[GAT ? 0 : u][q] + kj[q], a.slope), l[u]);
                    if (DOT) l[u] = fmaf(qq[GAT ? 0 : u][q], kj[q], l[u]);
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (!GAT) l[u] = group_sum<LPH>(l[u], a.lph);
                g[u] = group_sum<LPH>(g[u], a.lph);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                float lu = l[u];
                const float z = ln[u].w + ss;              // GAT
                if (GAT) lu = lrelu_w(z, a.slope);
                if (DOT) lu = lu / a.scale;
                float al = expf(lu - ln[u].x) * ln[u].y;
                al = (j + u < s.n) ? al : 0.0f;
                const float dl = al * (g[u] - ln[u].z);
                if (GAT) dss += z > 0.0f ? dl : dl * a.slope;
#pragma unroll
                for (int q = 0; q < VEC; ++q) {
                    dv[q] = fmaf(al, dd[u][q], dv[q]);
                    if (V2) {
                        const float sl = (qq[GAT ? 0 : u][q] + kj[q]) > 0.0f ? 1.0f : a.slope;
                        dk[q] = fmaf(dl * sl, r.ca[q], dk[q]);
                    }
                    if (DOT) dk[q] = fmaf(dl, qq[GAT ? 0 : u][q], dk[q]);
                }
            }
        }
    }
    if (!r.active) return;
    if (GAT) {
        float da[VEC];
#pragma unroll
        for (int q = 0; q < VEC; ++q) {
            dk[q] = fmaf(r.ca[q], dss, dv[q]);
            da[q] = dss * kj[q];
        }
        Vec<VEC>::store(a.dA + (int64_t)row * a.D + r.f0, da);
    }
    if (V2) {
#pragma unroll
        for (int q = 0; q < VEC; ++q) dk[q] = dk[q] + dv[q];    // V is K: one gradient
    }
    if (DOT) {
#pragma unroll
        for (int q = 0; q < VEC; ++q) dk[q] = dk[q] / a.scale;
        Vec<VEC>::store(a.dV + (int64_t)row * a.D + r.f0, dv);
    }
    if (a.fold) {                                          // Q is K: the destination half of the same row, from pass 1
        float dq[VEC];
        Vec<VEC>::load(a.dQ + (int64_t)row * a.D + r.f0, dq);
#pragma unroll
        for (int q = 0; q < VEC; ++q) dk[q] = dk[q] + dq[q];
    }
    Vec<VEC>::store(a.dK + (int64_t)row * a.D + r.f0, dk);
}

// da[(d / C) * ld + off + d % C] = Σ_i dA[i][d]: one block a column, thread k adds rows k, k + 256, ... in order, then a fixed tree — no
// scratch, equal bits; N = 0 gives the zero it should
__global__ void __launch_bounds__(256) attn_wide_da_kernel(const float *dA, float *da, int64_t N, int D, int C, int ld, int off) {
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
    if (threadIdx.x == 0) da[(d / C) * ld + off + d % C] = red[0];
}

// f(int_c<VEC>, int_c<LPH>, int_c<MODE>) for the tile geometry: DPP butterflies for every power-of-two head up to a whole wave
template <class F>
static void with_tile(const HeadTiles &ht, int mode, F &&f) {
    with_vec(ht.vec, [&](auto V) {
        with_lph<decltype(V)::value, 64>(ht.lph, [&](auto L) {
            if (mode == GNNMP_ATTN_GAT) f(V, L, int_c<GNNMP_ATTN_GAT>{});
            else if (mode == GNNMP_ATTN_GATV2) f(V, L, int_c<GNNMP_ATTN_GATV2>{});
            else f(V, L, int_c<GNNMP_ATTN_DOT>{});
        });
    });
}

}  // namespace gnnmp

using namespace gnnmp;

// The widest v every [.][H*C] array of a call admits (4 needs 16-byte, 2 needs 8-byte alignment of ALL of them; a null one admits any),
// narrowed to the head width, and the head tiles it gives
static HeadTiles wide_tiles(int64_t H, int64_t C, std::initializer_list<const float *> arrays) {
    uintptr_t align = 0;
    for (const float *p : arrays) align |= reinterpret_cast<uintptr_t>(p);
    return head_tiles(H, C, pick_vec(H * C, reinterpret_cast<const void *>(align), nullptr));
}

// what both exports check of (plan, job, mode, H, C) before anything else
static int attn_wide_check(const char *who, const gnnmp_graph_t *plan, const void *job, int mode, int64_t H, int64_t C) {
    if (!plan) return fail(GNNMP_EINVAL, "%s: null plan", who);
    if (!job) return fail(GNNMP_EINVAL, "%s: null job", who);
    if (mode == GNNMP_ATTN_COS) return fail(GNNMP_EUNSUPPORTED, "%s: the cosine logit is single-head: a head wider than a wave has no kernel", who);
    if (mode != GNNMP_ATTN_GAT && mode != GNNMP_ATTN_GATV2 && mode != GNNMP_ATTN_DOT) return fail(GNNMP_EINVAL, "%s: bad mode %d", who, mode);
    if (H <= 0 || C <= 0 || H > (1 << 20) || C > (1 << 20) || H * C > (1 << 20)) return fail(GNNMP_EINVAL, "%s: bad H/C", who);
    return GNNMP_OK;
}
static int wide_refuse_head(const char *who, int64_t C, const HeadTiles &ht) {
    return fail(GNNMP_EUNSUPPORTED, "%s: a head must fit one wave (C = %lld is %lld lanes of %d, at most 64)", who, (long long)C,
                (long long)(C / ht.vec), ht.vec);
}
static void wide_fill(AttnWideArgs &g, const HeadTiles &ht, int64_t H, int64_t C, float slope, float scale) {
    g.geom = RowGeom{6, 4, 0, 0};                          // one wave a (row, tile) whatever the knobs say: the tile IS the lane group
    g.H = (int)H;
    g.C = (int)C;
    g.D = (int)(H * C);
    g.lph = ht.lph_code;
    g.hpt = ht.hpt;
    g.slope = slope;
    g.scale = scale;
}

extern "C" int gnnmp_attn_conv_wide_f32(const gnnmp_graph_t *plan, int mode, const gnnmp_attn_wide_t *job, int64_t H, int64_t C,
                                        gnnmp_stream_t stream) {
    const char *who = "attn_conv_wide";
    GNNMP_TRY(attn_wide_check(who, plan, job, mode, H, C));
    if (job->act != GNNMP_ACT_IDENTITY && job->act != GNNMP_ACT_RELU) return fail(GNNMP_EINVAL, "%s: bad act %d", who, job->act);
    const float *Q = job->Q ? job->Q : job->K, *V = job->V ? job->V : job->K;
    if (mode != GNNMP_ATTN_DOT && V != job->K) return fail(GNNMP_EINVAL, "%s: a separate value array needs mode DOT", who);
    if (!job->out || !job->K || (mode != GNNMP_ATTN_DOT && !job->a)) return fail(GNNMP_EINVAL, "%s: null pointer", who);
    if (Q == job->K && plan->n_src != plan->n_dst) return fail(GNNMP_EINVAL, "%s: bipartite plan needs a separate Q", who);
    const HeadTiles ht = wide_tiles(H, C, {Q, job->K, V, job->out});
    if (!ht.fits) return wide_refuse_head(who, C, ht);
    if (plan->n_dst == 0) return GNNMP_OK;
    AttnWideArgs g = {};
    wide_fill(g, ht, H, C, job->negative_slope, job->scale);
    g.rows = plan_rows_whole(plan);
    g.Q = Q;
    g.K = job->K;
    g.V = V;
    g.a = job->a;
    g.bias = job->bias;
    g.out = job->out;
    g.stats = job->stats;
    g.act = job->act;
    dim3 grid;
    GNNMP_TRY(row_walk_grid(who, g.rows, g.geom, ht.tiles, grid));
    with_tile(ht, mode, [&](auto V_, auto L, auto M) {
        attn_wide_fwd_kernel<decltype(V_)::value, WIDE_U, decltype(L)::value, decltype(M)::value><<<grid, 256, 0, (hipStream_t)stream>>>(g);
    });
    GNNMP_LAUNCH_CHECK("attn_wide_fwd_kernel");
    return GNNMP_OK;
}

extern "C" int gnnmp_attn_conv_wide_grad_f32(const gnnmp_graph_t *plan, const gnnmp_graph_t *plan_t, int mode,
                                             const gnnmp_attn_wide_grad_t *job, int64_t H, int64_t C, gnnmp_stream_t stream) {
    const char *who = "attn_conv_wide_grad";
    GNNMP_TRY(attn_wide_check(who, plan, job, mode, H, C));
    if (!plan_t) return fail(GNNMP_EINVAL, "%s: null plan_t", who);
    GNNMP_TRY(check_transposed(who, plan, plan_t));
    const float *Q = job->Q ? job->Q : job->K, *V = job->V ? job->V : job->K;
    const bool gat = mode == GNNMP_ATTN_GAT, dot = mode == GNNMP_ATTN_DOT;
    if (!dot && V != job->K) return fail(GNNMP_EINVAL, "%s: a separate value array needs mode DOT", who);
    if (!job->K || !job->stats || !job->dout || !job->line || !job->dQ || !job->dK || (dot && !job->dV) || (!dot && (!job->a || !job->dA)))
        return fail(GNNMP_EINVAL, "%s: null pointer", who);
    if (Q == job->K && plan->n_src != plan->n_dst) return fail(GNNMP_EINVAL, "%s: bipartite plan needs a separate Q", who);
    if ((reinterpret_cast<uintptr_t>(job->line) & 15) != 0) return fail(GNNMP_EINVAL, "%s: line must be 16-byte aligned", who);
    const HeadTiles ht = wide_tiles(H, C, {Q, job->K, V, job->dout, job->dQ, job->dK, job->dV, job->dA});
    if (!ht.fits) return wide_refuse_head(who, C, ht);
    if (plan->n_dst == 0 && plan->n_src == 0) return GNNMP_OK;
    const hipStream_t st = (hipStream_t)stream;
    AttnWideArgs g = {};
    wide_fill(g, ht, H, C, job->negative_slope, job->scale);
    g.Q = Q;
    g.K = job->K;
    g.V = V;
    g.a = job->a;
    g.dout = job->dout;
    g.stats_in = job->stats;
    g.line = job->line;
    g.dQ = job->dQ;
    g.dA = job->dA;
    g.dK = job->dK;
    g.dV = job->dV;
    g.fold = Q == job->K;
    dim3 grid;
    g.rows = plan_rows_whole(plan);
    GNNMP_TRY(row_walk_grid(who, g.rows, g.geom, ht.tiles, grid));
    if (grid.x > 0) {
        with_tile(ht, mode, [&](auto V_, auto L, auto M) {
            attn_wide_bwd_dst_kernel<decltype(V_)::value, WIDE_U, decltype(L)::value, decltype(M)::value><<<grid, 256, 0, st>>>(g);
        });
        GNNMP_LAUNCH_CHECK("attn_wide_bwd_dst_kernel");
    }
    g.rows = plan_rows_whole(plan_t);
    if (gat) g.dA = job->dA + plan->n_dst * (H * C);        // GAT: the sources' terms follow the destinations'
    GNNMP_TRY(row_walk_grid(who, g.rows, g.geom, ht.tiles, grid));
    if (grid.x > 0) {
        with_tile(ht, mode, [&](auto V_, auto L, auto M) {
            attn_wide_bwd_src_kernel<decltype(V_)::value, WIDE_U, decltype(L)::value, decltype(M)::value><<<grid, 256, 0, st>>>(g);
        });
        GNNMP_LAUNCH_CHECK("attn_wide_bwd_src_kernel");
    }
    if (!dot && job->da) {
        const int D = g.D, Ci = (int)C;
        attn_wide_da_kernel<<<(unsigned)D, 256, 0, st>>>(job->dA, job->da, plan->n_dst, D, Ci, gat ? 2 * Ci : Ci, 0);
        if (gat) attn_wide_da_kernel<<<(unsigned)D, 256, 0, st>>>(g.dA, job->da, plan->n_src, D, Ci, 2 * Ci, Ci);
        GNNMP_LAUNCH_CHECK("attn_wide_da_kernel");
    }
    return GNNMP_OK;
}
