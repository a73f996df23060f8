// gat_backward.hip — adjoint of the one-pass GATConv attention path (gat_fused.hip; SURVEY.md §8f rank 1, "next").
// What Zygote differentiates in the reference (GNNlib/src/layers/conv.jl:136-141,152-167 + utils.jl:84-97), per head h:
//   z_ij = a_d.Wx_i + a_s.Wx_j     l_ij = leakyrelu(z_ij)     α_ij = softmax_{j in N(i)}(l_ij)     o_i = Σ_j α_ij Wx_j
// With Δ_i = dL/do_i [C] the chain rule collapses to
//   g_ij   = Δ_i . Wx_j                      D_i   = Σ_j α_ij g_ij                 (the softmax rrule's  Σ α dα)
//   dz_ij  = α_ij (g_ij - D_i) lrelu'(z_ij)  dsd_i = Σ_j dz_ij                     dss_j = Σ_i dz_ij
//   dWx_j  = Σ_i α_ij Δ_i  +  a_s dss_j  +  a_d dsd_j                             da_d = Σ_i dsd_i Wx_i,  da_s = Σ_j dss_j Wx_j
// The α are never stored (E' x H floats): the forward saves (m_i, den_i) per destination and head (gnnmp_gat_conv_stats_f32)
// and both kernels below rebuild α_ij = exp(l_ij - m_i) / den_i in registers, the same way the forward builds the logits.
//
//   gat_bwd_dst_kernel   destination-sorted plan (the forward's): one pass gathering Wx_j, three running sums per (i,h)
//                        S1 = Σ α g, S2 = Σ α g s, S3 = Σ α s  ->  D_i = S1,  dsd_i = S2 - S1 S3;  writes the 16-byte line
//                        (sd_i, m_i, 1/den_i, D_i) that the second kernel gathers per edge
//   gat_bwd_src_kernel   source-sorted plan (the transposed one): row j gathers Δ_i + that line for every edge that
//                        leaves j, accumulates Σ α Δ_i and dss_j, adds the two rank-one terms and stores dWx_j
//   da                   two weighted column sums over the nodes, deterministic slab partials (launch.h: column sums)
// Long rows are chunked into virtual rows exactly like the forward kernels; partials are folded in chunk order.
//
// Edge features (gnnmp_gat_conv_edge_grad_f32; conv.jl:152-167): z_ij gains es_k = a_e . We_k, one float per head at the slot's ORIGINAL
// edge position k (rows.eid, as DROP fetches it).  EDGE is a compile-time property of the two edge passes beside DROP: both add es_k to z
// before leakyrelu, the exponential and leakyrelu', and the source pass — where an edge is exactly one slot — stores des_k = dz_ij with
// one plain store.  The edge side needs no [E][H*C] array: with M[h][:] = Σ_c a_e[h][c] W_e[hC + c][:] (gat_edge_fold_kernel) es = e M',
// de = des M, dM = des' e are dense calls on the E rows of e, and gat_edge_fold_grad_kernel turns dM into dW_e and da_e.
#include <algorithm>
#include <type_traits>

#include "launch.h"
#include "rowwalk.h"

namespace gnnmp {

struct GatBwdArgs {
    PlanRows rows;        // of the plan the running pass walks (rows.eid: DROP's slot -> original edge position)
    const float *Wx_src;  // [n_src][D]
    const float *Wx_dst;  // [n_dst][D]
    const float *a;       // [H][2C]
    const float *dout;    // Δ [n_dst][D]
    const float *stats;   // [n_dst][H][2]  (m, den) from the forward
    float *line;          // [n_dst][H][4]  (sd, m, 1/den, D)
    float *dsd;           // [n_dst][H]
    float *dss;           // [n_src][H]
    float *dWx;           // [n_src][D]
    float *partial;
    int fold_dst;         // add a_d * dsd_j into dWx_j (non-bipartite: Wx_dst is Wx_src)
    int H, C, D, lph;
    RowGeom geom;
    float slope;
    DropArgs drop;
    // gnnmp_gat_conv_grad2_f32: what the training forward saved (gnnmp_gat_conv_train_f32) — the destination side then needs no edge pass
    const float *outk;    // [n_dst][D] the forward's output act(o + bias) with act in {identity, relu}
    const float *bias;    // [D] or null
    const float *oplus;   // [n_dst][D]
    const float *pplus;   // [n_dst][H]
};
// what the EDGE instances take (gnnmp_gat_conv_edge_grad_f32).  A type of its own: the kernel arguments of the e-less instances, and with
// them their code, stay what they were
struct GatBwdEdgeArgs : GatBwdArgs {
    const float *escore;  // [n_edges][H] es_k, original edge order
    float *dscore;        // [n_edges][H] des_k = dz_ij
};
template <bool EDGE>
using GatBwdArgsOf = std::conditional_t<EDGE, GatBwdEdgeArgs, GatBwdArgs>;

__device__ __forceinline__ float lrelu_b(float x, float slope) { return x > 0.0f ? x : x * slope; }

template <int VEC, int U, int LPH, bool DROP, bool EDGE = false>
__global__ void __launch_bounds__(256) gat_bwd_dst_kernel(const GatBwdArgsOf<EDGE> a) {
    VRow vr;
    if (!decode_vrow(a.rows, a.geom, blockIdx.x, vr)) return;
    const int v = vr.v, row = vr.row, lig = vr.lig, gbase = vr.gbase, G = vr.G;
    const bool is_chunk = vr.is_chunk;
    const uint32_t beg = vr.beg, end = vr.end;
    const int f0 = lig * VEC;
    const bool active = f0 < a.D;
    const int fc = active ? f0 : 0;   // idle lanes (D/VEC not a power of two) shadow lane 0 with zero coefficients
    const int h = fc / a.C;
    float ad[VEC], as[VEC], vi[VEC], di[VEC];
    {
        const float *ah = a.a + (int64_t)h * 2 * a.C + (fc - h * a.C);
#pragma unroll
        for (int q = 0; q < VEC; ++q) {
            ad[q] = active ? ah[q] : 0.0f;
            as[q] = active ? ah[a.C + q] : 0.0f;
        }
    }
    Vec<VEC>::load(a.Wx_dst + (int64_t)row * a.D + fc, vi);
    Vec<VEC>::load(a.dout + (int64_t)row * a.D + fc, di);
#pragma unroll
    for (int q = 0; q < VEC; ++q) di[q] = active ? di[q] : 0.0f;   // H = 1: idle lanes sit inside the head's butterfly
    float sd = 0.0f;
#pragma unroll
    for (int q = 0; q < VEC; ++q) sd = fmaf(ad[q], vi[q], sd);
    sd = group_sum<LPH>(sd, a.lph);
    const float m = a.stats[((int64_t)row * a.H + h) * 2];
    const float den = a.stats[((int64_t)row * a.H + h) * 2 + 1];
    const float rden = 1.0f / den;

    // branch-free body: the U loads, the 2U dot products, their butterflies and the U exponentials are independent
    // chains the scheduler interleaves; slots past the end of the row re-read the last edge and get α = 0
    float S1 = 0.0f, S2 = 0.0f, S3 = 0.0f;
    for (uint32_t base = beg; base < end; base += G) {   // slots are unsigned 32-bit (rowwalk.h)
        const uint32_t p = base + lig;
        const int c = p < end ? a.rows.col[p] : 0;
        const int ev = ((DROP || EDGE) && p < end) ? a.rows.eid[p] : 0;
        const int n = (int)min((uint32_t)G, end - base);
        for (int j = 0; j < n; j += U) {
            float w[U][VEC];
            float kf[DROP ? U : 1];      // keep_ij / (1 - p) of conv.jl:139's dropout (common.h drop_bits): g_ij becomes kf g_ij
            float es[EDGE ? U : 1];      // the edge's share of the logit, from the slot's original edge position
            (void)es;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int cj = __shfl(c, gbase + min(j + u, n - 1), 64);
                Vec<VEC>::load(a.Wx_src + (int64_t)cj * a.D + fc, w[u]);
                if (DROP) {
                    const uint32_t ej = (uint32_t)__shfl(ev, gbase + min(j + u, n - 1), 64);
                    kf[DROP ? u : 0] = drop_bits(a.drop.seed_lo, a.drop.seed_hi, ej, (uint32_t)h) >= a.drop.thr ? a.drop.inv : 0.0f;
                }
                if constexpr (EDGE) {
                    const uint32_t ej = (uint32_t)__shfl(ev, gbase + min(j + u, n - 1), 64);
                    es[u] = a.escore[(int64_t)ej * a.H + h];
                }
            }
            float d[U], g[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                d[u] = 0.0f;
                g[u] = 0.0f;
#pragma unroll
                for (int q = 0; q < VEC; ++q) {
                    d[u] = fmaf(as[q], w[u][q], d[u]);
                    g[u] = fmaf(di[q], w[u][q], g[u]);
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                d[u] = group_sum<LPH>(d[u], a.lph);
                g[u] = group_sum<LPH>(g[u], a.lph);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const float z = EDGE ? (sd + d[u]) + es[EDGE ? u : 0] : sd + d[u];   // the forward's order: (target + source) + edge
                float al = expf(lrelu_b(z, a.slope) - m) * rden;
                al = (j + u < n) ? al : 0.0f;
                const float s = z > 0.0f ? 1.0f : a.slope;
                const float ag = DROP ? al * (kf[DROP ? u : 0] * g[u]) : al * g[u];
                S1 += ag;
                S2 = fmaf(ag, s, S2);
                S3 = fmaf(al, s, S3);
            }
        }
    }
    if (!active || (f0 % a.C) != 0) return;
    if (is_chunk) {
        float *pc = a.partial + ((int64_t)v * a.H + h) * 4;
        pc[0] = S1;
        pc[1] = S2;
        pc[2] = S3;
        pc[3] = sd;
        return;
    }
    float *ln = a.line + ((int64_t)row * a.H + h) * 4;
    ln[0] = sd;
    ln[1] = m;
    ln[2] = end > beg ? rden : 0.0f;
    ln[3] = S1;
    a.dsd[(int64_t)row * a.H + h] = S2 - S1 * S3;
}

// The destination side WITHOUT an edge pass (round 4).  With o_i = Σ_j α_ij Wx_j (the forward's output before bias and σ):
//   D_i = Σ_j α_ij g_ij = Δ_i . o_i                                   (g_ij = Δ_i . Wx_j is linear in Wx_j)
//   dsd_i = Σ_j α_ij (g_ij - D_i) lrelu'(z_ij),  lrelu' = slope + (1 - slope) [z_ij > 0]
//         = slope D_i + (1 - slope) Δ_i . o+_i - D_i (slope + (1 - slope) P_i) = (1 - slope) (Δ_i . o+_i - D_i P_i)
// o+_i / P_i = the same sums over the edges with z_ij > 0 only: the training forward accumulates them next to o_i (gat_fused.hip,
// ATTN_GAT_PLUS).  o_i is read back from the forward's output act(o_i + b): on entries that relu switched off Δ is zero (the caller
// passes dL/d(o + b)), elsewhere o = out - b.  One lane group per row, three row loads, three butterflies: 3.8 GB instead of the
// 5.7 ms gather of every Wx_j.
template <int VEC, int LPH>
__global__ void __launch_bounds__(256) gat_bwd_node_kernel(const GatBwdArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int G = 1 << a.geom.log2g;
    const int lig = lane & (G - 1);
    const int grp = lane >> a.geom.log2g;
    const int rpw = 64 >> a.geom.log2g;
    const int64_t r64 = ((int64_t)blockIdx.x * (blockDim.x >> 6) + wave) * rpw + grp;
    if (r64 >= a.rows.n_rows) return;
    const int row = (int)r64;
    const int f0 = lig * VEC;
    const bool active = f0 < a.D;
    const int fc = active ? f0 : 0;
    const int h = fc / a.C;
    float vi[VEC], di[VEC], ok[VEC], op[VEC];
    Vec<VEC>::load(a.Wx_dst + (int64_t)row * a.D + fc, vi);
    Vec<VEC>::load(a.dout + (int64_t)row * a.D + fc, di);
    Vec<VEC>::load(a.outk + (int64_t)row * a.D + fc, ok);
    Vec<VEC>::load(a.oplus + (int64_t)row * a.D + fc, op);
    const float *ah = a.a + (int64_t)h * 2 * a.C + (fc - h * a.C);
    float sd = 0.0f, Dv = 0.0f, Tv = 0.0f;
#pragma unroll
    for (int q = 0; q < VEC; ++q) {
        const float d = active ? di[q] : 0.0f;
        const float o = ok[q] - (a.bias ? a.bias[fc + q] : 0.0f);
        sd = fmaf(active ? ah[q] : 0.0f, vi[q], sd);
        Dv = fmaf(d, o, Dv);
        Tv = fmaf(d, op[q], Tv);
    }
    sd = group_sum<LPH>(sd, a.lph);
    Dv = group_sum<LPH>(Dv, a.lph);
    Tv = group_sum<LPH>(Tv, a.lph);
    if (!active || (f0 % a.C) != 0) return;
    const float m = a.stats[((int64_t)row * a.H + h) * 2];
    const float den = a.stats[((int64_t)row * a.H + h) * 2 + 1];
    const bool any = a.rows.rowptr[row + 1] > a.rows.rowptr[row];
    float *ln = a.line + ((int64_t)row * a.H + h) * 4;
    ln[0] = sd;
    ln[1] = m;
    ln[2] = any ? 1.0f / den : 0.0f;
    ln[3] = any ? Dv : 0.0f;
    a.dsd[(int64_t)row * a.H + h] = any ? (1.0f - a.slope) * (Tv - Dv * a.pplus[(int64_t)row * a.H + h]) : 0.0f;
}

__global__ void __launch_bounds__(256) gat_bwd_dst_combine_kernel(const GatBwdArgs a) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)a.rows.n_long * a.H) return;
    const int r = (int)(i / a.H), h = (int)(i - (int64_t)r * a.H);
    const int row = a.rows.long_rows[r];
    const int c0 = a.rows.long_cptr[r], c1 = a.rows.long_cptr[r + 1];
    float S1 = 0.0f, S2 = 0.0f, S3 = 0.0f;
    for (int c = c0; c < c1; ++c) {
        const float *pc = a.partial + ((int64_t)c * a.H + h) * 4;
        S1 += pc[0];
        S2 += pc[1];
        S3 += pc[2];
    }
    float *ln = a.line + ((int64_t)row * a.H + h) * 4;
    ln[0] = a.partial[((int64_t)c0 * a.H + h) * 4 + 3];
    ln[1] = a.stats[((int64_t)row * a.H + h) * 2];
    ln[2] = 1.0f / a.stats[((int64_t)row * a.H + h) * 2 + 1];
    ln[3] = S1;
    a.dsd[(int64_t)row * a.H + h] = S2 - S1 * S3;
}

template <int VEC>
__device__ __forceinline__ void gat_bwd_src_store(const GatBwdArgs &a, int row, int f0, int h, const float as[VEC],
                                                  const float ad[VEC], float acc[VEC], float dss) {
    float extra = 0.0f;
    if (a.fold_dst) extra = a.dsd[(int64_t)row * a.H + h];
#pragma unroll
    for (int q = 0; q < VEC; ++q) {
        acc[q] = fmaf(as[q], dss, acc[q]);
        if (a.fold_dst) acc[q] = fmaf(ad[q], extra, acc[q]);
    }
    Vec<VEC>::store(a.dWx + (int64_t)row * a.D + f0, acc);
    if ((f0 % a.C) == 0) a.dss[(int64_t)row * a.H + h] = dss;
}

template <int VEC, int U, int LPH, bool DROP, bool EDGE = false>
__global__ void __launch_bounds__(256) gat_bwd_src_kernel(const GatBwdArgsOf<EDGE> a) {
    VRow vr;
    if (!decode_vrow(a.rows, a.geom, blockIdx.x, vr)) return;
    const int v = vr.v, row = vr.row, lig = vr.lig, gbase = vr.gbase, G = vr.G;
    const bool is_chunk = vr.is_chunk;
    const uint32_t beg = vr.beg, end = vr.end;
    const int f0 = lig * VEC;
    const bool active = f0 < a.D;
    const int fc = active ? f0 : 0;
    const int h = fc / a.C;
    float ad[VEC], as[VEC], wj[VEC];
    {
        const float *ah = a.a + (int64_t)h * 2 * a.C + (fc - h * a.C);
#pragma unroll
        for (int q = 0; q < VEC; ++q) {
            ad[q] = active ? ah[q] : 0.0f;
            as[q] = active ? ah[a.C + q] : 0.0f;
        }
    }
    Vec<VEC>::load(a.Wx_src + (int64_t)row * a.D + fc, wj);
#pragma unroll
    for (int q = 0; q < VEC; ++q) wj[q] = active ? wj[q] : 0.0f;   // H = 1: idle lanes sit inside the head's butterfly
    float ss = 0.0f;
#pragma unroll
    for (int q = 0; q < VEC; ++q) ss = fmaf(as[q], wj[q], ss);
    ss = group_sum<LPH>(ss, a.lph);

    float acc[VEC], dss = 0.0f;
#pragma unroll
    for (int q = 0; q < VEC; ++q) acc[q] = 0.0f;
    for (uint32_t base = beg; base < end; base += G) {   // slots are unsigned 32-bit (rowwalk.h)
        const uint32_t p = base + lig;
        const int c = p < end ? a.rows.col[p] : 0;
        const int ev = ((DROP || EDGE) && p < end) ? a.rows.eid[p] : 0;
        const int n = (int)min((uint32_t)G, end - base);
        for (int j = 0; j < n; j += U) {
            float dv[U][VEC];
            float4 ln[U];
            float kf[DROP ? U : 1];
            float es[EDGE ? U : 1];
            int64_t ek[EDGE ? U : 1];    // where des_k goes: [original edge position][h]
            (void)es;
            (void)ek;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int ci = __shfl(c, gbase + min(j + u, n - 1), 64);
                Vec<VEC>::load(a.dout + (int64_t)ci * a.D + fc, dv[u]);
                ln[u] = *reinterpret_cast<const float4 *>(a.line + ((int64_t)ci * a.H + h) * 4);
                if (DROP) {    // (the transposed plan's slots carry the same original edge positions)
                    const uint32_t ej = (uint32_t)__shfl(ev, gbase + min(j + u, n - 1), 64);
                    kf[DROP ? u : 0] = drop_bits(a.drop.seed_lo, a.drop.seed_hi, ej, (uint32_t)h) >= a.drop.thr ? a.drop.inv : 0.0f;
                }
                if constexpr (EDGE) {
                    const uint32_t ej = (uint32_t)__shfl(ev, gbase + min(j + u, n - 1), 64);
                    ek[u] = (int64_t)ej * a.H + h;
                    es[u] = a.escore[ek[u]];
                }
            }
            float g[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                g[u] = 0.0f;
#pragma unroll
                for (int q = 0; q < VEC; ++q) g[u] = fmaf(dv[u][q], wj[q], g[u]);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) g[u] = group_sum<LPH>(g[u], a.lph);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const float z = EDGE ? (ln[u].x + ss) + es[EDGE ? u : 0] : ln[u].x + ss;
                float al = expf(lrelu_b(z, a.slope) - ln[u].y) * ln[u].z;
                al = (j + u < n) ? al : 0.0f;
                const float s = z > 0.0f ? 1.0f : a.slope;
                const float gk = DROP ? kf[DROP ? u : 0] * g[u] : g[u];
                // des_k = dz_ij: an edge is exactly one slot of this plan, so one lane of the head stores it once, chunk or whole row alike
                if constexpr (EDGE) {
                    if (j + u < n && active && (f0 % a.C) == 0) a.dscore[ek[u]] = (al * (gk - ln[u].w)) * s;
                }
                dss = fmaf(al * (gk - ln[u].w), s, dss);
                const float ak = DROP ? al * kf[DROP ? u : 0] : al;
#pragma unroll
                for (int q = 0; q < VEC; ++q) acc[q] = fmaf(ak, dv[u][q], acc[q]);
            }
        }
    }
    if (!active) return;
    if (is_chunk) {
        const int LN = a.D / VEC;
        float *pc = a.partial + (int64_t)v * (a.D + LN);
        Vec<VEC>::store(pc + f0, acc);
        pc[a.D + f0 / VEC] = dss;
        return;
    }
    gat_bwd_src_store<VEC>(a, row, f0, h, as, ad, acc, dss);
}

template <int VEC>
__global__ void __launch_bounds__(256) gat_bwd_src_combine_kernel(const GatBwdArgs a) {
    const int G = 1 << a.geom.log2g;
    const int lig = threadIdx.x & (G - 1);
    const int64_t r = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> a.geom.log2g;
    if (r >= a.rows.n_long) return;
    const int f0 = lig * VEC;
    if (f0 >= a.D) return;
    const int h = f0 / a.C;
    const int row = a.rows.long_rows[r];
    const int c0 = a.rows.long_cptr[r], c1 = a.rows.long_cptr[r + 1];
    const int LN = a.D / VEC;
    const int64_t S = a.D + LN;
    constexpr int CB = 8;
    float acc[VEC], dss = 0.0f;
#pragma unroll
    for (int q = 0; q < VEC; ++q) acc[q] = 0.0f;
    for (int c = c0; c < c1; c += CB) {
        float sv[CB], pv[CB][VEC];
#pragma unroll
        for (int u = 0; u < CB; ++u) {
            const float *pc = a.partial + (int64_t)min(c + u, c1 - 1) * S;
            sv[u] = pc[a.D + f0 / VEC];
            Vec<VEC>::load(pc + f0, pv[u]);
        }
#pragma unroll
        for (int u = 0; u < CB; ++u) {
            if (c + u < c1) {
                dss += sv[u];
#pragma unroll
                for (int q = 0; q < VEC; ++q) acc[q] += pv[u][q];
            }
        }
    }
    float ad[VEC], as[VEC];
    const float *ah = a.a + (int64_t)h * 2 * a.C + (f0 - h * a.C);
#pragma unroll
    for (int q = 0; q < VEC; ++q) {
        ad[q] = ah[q];
        as[q] = ah[a.C + q];
    }
    gat_bwd_src_store<VEC>(a, row, f0, h, as, ad, acc, dss);
}

// dWx_dst[i][h][c] = a_d[h][c] * dsd[i][h]   (bipartite layers only: otherwise folded into gat_bwd_src_kernel)
__global__ void __launch_bounds__(256) gat_bwd_dst_rows_kernel(const float *a, const float *dsd, float *out, int64_t n,
                                                               int H, int C) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int D = H * C;
    if (i >= n * D) return;
    const int64_t r = i / D;
    const int f = (int)(i - r * D), h = f / C;
    out[i] = a[(int64_t)h * 2 * C + (f - h * C)] * dsd[r * H + h];
}

// M[h][k] = Σ_c a_e[h][c] W_e[hC + c][k]: the edge projection folded through the edge third of `a` — es = e M' then is one dense call
// on the E rows of e, and no [E][H*C] array exists in training.  One thread an element, c in order.
__global__ void __launch_bounds__(256) gat_edge_fold_kernel(const float *a_e, const float *W_e, float *M, int H, int C, int64_t ein) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)H * ein) return;
    const int h = (int)(i / ein);
    const int64_t k = i - (int64_t)h * ein;
    float acc = 0.0f;
    for (int c = 0; c < C; ++c) acc = fmaf(a_e[(int64_t)h * C + c], W_e[((int64_t)h * C + c) * ein + k], acc);
    M[i] = acc;
}
// its pullback: dW_e[hC + c][k] = a_e[h][c] dM[h][k] and da_e[h][c] = Σ_k dM[h][k] W_e[hC + c][k] — one thread a row of W_e, k in order
__global__ void __launch_bounds__(256) gat_edge_fold_grad_kernel(const float *a_e, const float *W_e, const float *dM, float *dW_e,
                                                                 float *da_e, int H, int C, int64_t ein) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= (int64_t)H * C) return;
    const int64_t h = r / C;
    const float ar = a_e[r];
    float acc = 0.0f;
    for (int64_t k = 0; k < ein; ++k) {
        const float d = dM[h * ein + k];
        if (dW_e) dW_e[r * ein + k] = ar * d;
        acc = fmaf(d, W_e[r * ein + k], acc);
    }
    if (da_e) da_e[r] = acc;
}

template <int VEC, int LPH, bool DROP, bool EDGE = false>
static int launch_gat_bwd(GatBwdArgsOf<EDGE> g, gnnmp_graph *plan, gnnmp_graph *plan_t, float *dWx_dst, float *da,
                          hipStream_t stream) {
    const int rpw = 64 >> g.geom.log2g;
    const int waves = block_waves(1);
    g.geom.waves = waves;
    const int unroll = knob(KNOB_UNROLL);
    // ---- pass 1: destinations (forward plan)
    g.rows = plan_rows(plan);
    g.partial = plan->ws;
    if (g.oplus) {        // the training forward saved o+ / P: a node kernel, no edge pass
        const int64_t blocks = ((int64_t)g.rows.n_rows + (int64_t)rpw * 4 - 1) / ((int64_t)rpw * 4);
        if (blocks > 0) {
            gat_bwd_node_kernel<VEC, LPH><<<(unsigned)blocks, 256, 0, stream>>>(g);
            GNNMP_LAUNCH_CHECK("gat_bwd_node_kernel");
        }
    } else {
        const unsigned blocks = row_grid(g.rows, g.geom, 1).x;
        if (blocks > 0) {
            if (unroll == 4)
                gat_bwd_dst_kernel<VEC, 4, LPH, DROP, EDGE><<<blocks, 64 * waves, 0, stream>>>(g);
            else
                gat_bwd_dst_kernel<VEC, 8, LPH, DROP, EDGE><<<blocks, 64 * waves, 0, stream>>>(g);
            GNNMP_LAUNCH_CHECK("gat_bwd_dst_kernel");
        }
        if (g.rows.n_long > 0) {
            const int64_t threads = (int64_t)g.rows.n_long * g.H;
            gat_bwd_dst_combine_kernel<<<(unsigned)((threads + 255) / 256), 256, 0, stream>>>(g);
            GNNMP_LAUNCH_CHECK("gat_bwd_dst_combine_kernel");
        }
    }
    // ---- pass 2: sources (transposed plan)
    g.rows = plan_rows(plan_t);
    g.partial = plan_t->ws;
    {
        const unsigned blocks = row_grid(g.rows, g.geom, 1).x;
        if (blocks > 0) {
            // 20 bytes of operands per lane and edge here (Δ slice + the statistics line): 4 in flight keeps 6 waves/SIMD
            // (7.0 ms on the products shape against 8.4 ms with 8 in flight at 4 waves/SIMD)
            if (unroll == 8)
                gat_bwd_src_kernel<VEC, 8, LPH, DROP, EDGE><<<blocks, 64 * waves, 0, stream>>>(g);
            else
                gat_bwd_src_kernel<VEC, 4, LPH, DROP, EDGE><<<blocks, 64 * waves, 0, stream>>>(g);
            GNNMP_LAUNCH_CHECK("gat_bwd_src_kernel");
        }
        if (g.rows.n_long > 0) {
            const int64_t threads = (int64_t)g.rows.n_long << g.geom.log2g;
            gat_bwd_src_combine_kernel<VEC><<<(unsigned)((threads + 255) / 256), 256, 0, stream>>>(g);
            GNNMP_LAUNCH_CHECK("gat_bwd_src_combine_kernel");
        }
    }
    // ---- rank-one target term for bipartite layers
    if (dWx_dst) {
        const int64_t n = (int64_t)plan->n_dst * g.D;
        gat_bwd_dst_rows_kernel<<<(unsigned)((n + 255) / 256), 256, 0, stream>>>(g.a, g.dsd, dWx_dst, plan->n_dst, g.H, g.C);
        GNNMP_LAUNCH_CHECK("gat_bwd_dst_rows_kernel");
    }
    // ---- da (both plans' chunk partials are dead by now in stream order: reuse the forward plan's workspace)
    if (da) {
        for (int side = 0; side < 2; ++side) {
            const float *x = side == 0 ? g.Wx_dst : g.Wx_src;
            const float *s = side == 0 ? g.dsd : g.dss;
            const int64_t N = side == 0 ? plan->n_dst : plan->n_src;
            const int nparts = colsum_parts(N);
            GNNMP_TRY(colsum_partial(x, s, N, g.D, g.C, colsum_slab_rows(N), nparts, plan->ws, stream));
            GNNMP_TRY(colsum_tree_fold(plan->ws, nparts, g.D, g.C, 2 * g.C, side * g.C, da, stream));
        }
    }
    return GNNMP_OK;
}

}  // namespace gnnmp

using namespace gnnmp;

// one call of GATConv's pullback: what the three exports below ask of gat_conv_grad_impl, by name
struct GatGradCall {
    const float *Wx_src = nullptr, *Wx_dst = nullptr, *a = nullptr;
    float negative_slope = 0.0f;
    float drop_p = 0.0f;
    uint64_t drop_seed = 0;
    const float *stats = nullptr, *dout = nullptr;
    float *line = nullptr, *dsd = nullptr, *dss = nullptr, *dWx_src = nullptr, *dWx_dst = nullptr, *da = nullptr;
    int64_t H = 0, C = 0;
    // grad2 (after gnnmp_gat_conv_train_f32): the forward's out, its bias, o+ and P
    const float *outk = nullptr, *bias = nullptr, *oplus = nullptr, *pplus = nullptr;
    // gnnmp_gat_conv_edge_grad_f32: the per-edge logit term and its gradient (both null on a plan without edges)
    bool edge = false;
    const float *escore = nullptr;
    float *dscore = nullptr;
};

static int gat_conv_grad_impl(gnnmp_graph_t *plan, gnnmp_graph_t *plan_t, GatGradCall c, gnnmp_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (c.edge && (c.oplus || c.drop_p > 0.0f)) return fail(GNNMP_EINVAL, "gat_conv_edge_grad: no dropout and no o+ / P shortcut together with edge features");
    if (c.oplus && (!c.outk || !c.pplus || c.drop_p > 0.0f)) return fail(GNNMP_EINVAL, "gat_conv_grad2: needs out, oplus and pplus of gnnmp_gat_conv_train_f32");
    if (!(c.drop_p >= 0.0f && c.drop_p < 1.0f)) return fail(GNNMP_EINVAL, "gat_conv_grad: dropout probability %g outside [0, 1)", (double)c.drop_p);
    if (!plan || !plan_t) return fail(GNNMP_EINVAL, "gat_conv_grad: null plan");
    if (c.H <= 0 || c.C <= 0 || c.H * c.C > (1 << 20)) return fail(GNNMP_EINVAL, "gat_conv_grad: bad H/C");
    GNNMP_TRY(check_transposed("gat_conv_grad", plan, plan_t));
    const bool same = !c.Wx_dst || c.Wx_dst == c.Wx_src;
    if (same) c.Wx_dst = c.Wx_src;
    if (same && plan->n_src != plan->n_dst) return fail(GNNMP_EINVAL, "gat_conv_grad: bipartite plan needs Wx_dst");
    if (!same && !c.dWx_dst) return fail(GNNMP_EINVAL, "gat_conv_grad: separate Wx_dst needs dWx_dst");
    if (same && c.dWx_dst) return fail(GNNMP_EINVAL, "gat_conv_grad: dWx_dst given but Wx_dst is Wx_src (the target term is folded into dWx_src)");
    if (plan->n_dst == 0 && plan->n_src == 0) return GNNMP_OK;
    if (!c.Wx_src || !c.a || !c.stats || !c.dout || !c.line || !c.dsd || !c.dss || !c.dWx_src)
        return fail(GNNMP_EINVAL, "gat_conv_grad: null pointer");
    const int D = (int)(c.H * c.C);
    // every array read or written with Vec<VEC> enters the decision (grad2's out / oplus included: an under-aligned one narrows the
    // lanes like any other array, the header promises alignment for `line` only); dWx_dst is written by a scalar kernel
    const HeadGeom hg = head_geom(c.H, c.C, narrow_vec(pick_vec(D, c.Wx_src, c.dWx_src), c.Wx_dst, c.dout, c.outk, c.oplus));
    if ((reinterpret_cast<uintptr_t>(c.line) & 15) != 0) return fail(GNNMP_EINVAL, "gat_conv_grad: line must be 16-byte aligned");
    if (!hg.fits_wave)
        return fail(GNNMP_EUNSUPPORTED, "gat_conv_grad: the feature row must fit one wave (H*C = %lld)", (long long)(c.H * c.C));
    // workspaces: chunk partials of each pass in that plan's workspace; the da partials reuse the forward plan's
    const size_t colsum_need = (size_t)std::max(colsum_parts(plan->n_dst), colsum_parts(plan->n_src)) * (size_t)D;
    if (int rc = ensure_workspace(plan, std::max((size_t)plan->n_chunks * (size_t)c.H * 4, c.da ? colsum_need : (size_t)0))) return rc;
    if (plan_t->n_chunks > 0)
        if (int rc = ensure_workspace(plan_t, (size_t)plan_t->n_chunks * (size_t)(D + hg.lanes))) return rc;
    GatBwdArgs g;
    g.Wx_src = c.Wx_src;
    g.Wx_dst = c.Wx_dst;
    g.a = c.a;
    g.dout = c.dout;
    g.stats = c.stats;
    g.line = c.line;
    g.dsd = c.dsd;
    g.dss = c.dss;
    g.dWx = c.dWx_src;
    g.fold_dst = same ? 1 : 0;
    g.H = (int)c.H;
    g.C = (int)c.C;
    g.D = D;
    g.geom = RowGeom{hg.log2g, 1, 0, 0};
    g.lph = hg.lph_code;
    g.slope = c.negative_slope;
    g.drop = make_drop(c.drop_p, c.drop_seed);
    g.outk = c.outk;
    g.bias = c.bias;
    g.oplus = c.oplus;
    g.pplus = c.pplus;
    return with_vec(hg.vec, [&](auto V) {
        constexpr int VEC = decltype(V)::value;
        if (c.edge) {
            GatBwdEdgeArgs ge;
            static_cast<GatBwdArgs &>(ge) = g;
            ge.escore = c.escore;
            ge.dscore = c.dscore;
            return with_lph<VEC, 16>(hg.lph, [&](auto L) { return launch_gat_bwd<VEC, decltype(L)::value, false, true>(ge, plan, plan_t, c.dWx_dst, c.da, stream); });
        }
        // the dropout variants walk the head butterfly with the run-time lane count (one instantiation per width)
        if (c.drop_p > 0.0f) return launch_gat_bwd<VEC, 0, true>(g, plan, plan_t, c.dWx_dst, c.da, stream);
        // the usual case (C a multiple of 4): compile-time lane count per head -> DPP butterflies
        return with_lph<VEC, 16>(hg.lph, [&](auto L) { return launch_gat_bwd<VEC, decltype(L)::value, false>(g, plan, plan_t, c.dWx_dst, c.da, stream); });
    });
}

// what the three exports share (their arguments in the exports' order)
static GatGradCall gat_grad_call(const float *Wx_src, const float *Wx_dst, const float *a, float negative_slope, const float *stats,
                                 const float *dout, float *line, float *dsd, float *dss, float *dWx_src, float *dWx_dst, float *da,
                                 int64_t H, int64_t C) {
    GatGradCall c;
    c.Wx_src = Wx_src;
    c.Wx_dst = Wx_dst;
    c.a = a;
    c.negative_slope = negative_slope;
    c.stats = stats;
    c.dout = dout;
    c.line = line;
    c.dsd = dsd;
    c.dss = dss;
    c.dWx_src = dWx_src;
    c.dWx_dst = dWx_dst;
    c.da = da;
    c.H = H;
    c.C = C;
    return c;
}

extern "C" int gnnmp_gat_conv_grad_f32(gnnmp_graph_t *plan, gnnmp_graph_t *plan_t, const float *Wx_src,
                                       const float *Wx_dst, const float *a, float negative_slope, const float *stats,
                                       const float *dout, float *line, float *dsd, float *dss, float *dWx_src,
                                       float *dWx_dst, float *da, int64_t H, int64_t C, gnnmp_stream_t stream) {
    return gat_conv_grad_impl(plan, plan_t, gat_grad_call(Wx_src, Wx_dst, a, negative_slope, stats, dout, line, dsd, dss, dWx_src, dWx_dst, da, H, C),
                              stream);
}
extern "C" int gnnmp_gat_conv_grad_drop_f32(gnnmp_graph_t *plan, gnnmp_graph_t *plan_t, const float *Wx_src,
                                            const float *Wx_dst, const float *a, float negative_slope, float p, uint64_t seed,
                                            const float *stats, const float *dout, float *line, float *dsd, float *dss,
                                            float *dWx_src, float *dWx_dst, float *da, int64_t H, int64_t C,
                                            gnnmp_stream_t stream) {
    GatGradCall c = gat_grad_call(Wx_src, Wx_dst, a, negative_slope, stats, dout, line, dsd, dss, dWx_src, dWx_dst, da, H, C);
    c.drop_p = p;
    c.drop_seed = seed;
    return gat_conv_grad_impl(plan, plan_t, c, stream);
}

/* The pullback after gnnmp_gat_conv_train_f32 (see gnnmp.h): the destination side is a node kernel on (Δ, out, o+, P), one edge pass
 * (the source side) instead of two */
extern "C" int gnnmp_gat_conv_grad2_f32(gnnmp_graph_t *plan, gnnmp_graph_t *plan_t, const float *Wx_src, const float *Wx_dst,
                                        const float *a, float negative_slope, const float *stats, const float *out, const float *bias,
                                        const float *oplus, const float *pplus, const float *dout, float *line, float *dsd, float *dss,
                                        float *dWx_src, float *dWx_dst, float *da, int64_t H, int64_t C, gnnmp_stream_t stream) {
    if (!out || !oplus || !pplus) return fail(GNNMP_EINVAL, "gat_conv_grad2: null out / oplus / pplus");
    GatGradCall c = gat_grad_call(Wx_src, Wx_dst, a, negative_slope, stats, dout, line, dsd, dss, dWx_src, dWx_dst, da, H, C);
    c.outk = out;
    c.bias = bias;
    c.oplus = oplus;
    c.pplus = pplus;
    return gat_conv_grad_impl(plan, plan_t, c, stream);
}

/* GATConv's pullback with edge features (see gnnmp.h): the two edge passes with the per-edge logit term, des written by the source pass */
extern "C" int gnnmp_gat_conv_edge_grad_f32(gnnmp_graph_t *plan, gnnmp_graph_t *plan_t, const gnnmp_gat_edge_grad_t *job, int64_t H,
                                            int64_t C, gnnmp_stream_t stream) {
    if (!plan || !plan_t) return fail(GNNMP_EINVAL, "gat_conv_edge_grad: null plan");
    if (!job) return fail(GNNMP_EINVAL, "gat_conv_edge_grad: null job");
    if (plan->self_loops || plan->n_total != plan->n_edges)
        return fail(GNNMP_EINVAL, "gat_conv_edge_grad: the plan was built with self loops (%lld slots, %lld edges): edge_score has no row for them "
                                  "(GNNlib/src/layers/conv.jl:119-121)", (long long)plan->n_total, (long long)plan->n_edges);
    if (plan->n_edges > 0 && (!job->edge_score || !job->dscore)) return fail(GNNMP_EINVAL, "gat_conv_edge_grad: null edge_score / dscore");
    GatGradCall c = gat_grad_call(job->Wx_src, job->Wx_dst, job->a, job->negative_slope, job->stats, job->dout, job->line, job->dsd, job->dss,
                                  job->dWx_src, job->dWx_dst, job->da, H, C);
    c.edge = true;
    c.escore = job->edge_score;
    c.dscore = job->dscore;
    return gat_conv_grad_impl(plan, plan_t, c, stream);
}

extern "C" int gnnmp_gat_edge_fold_f32(const float *a_e, const float *W_e, float *M, int64_t H, int64_t C, int64_t ein, gnnmp_stream_t stream) {
    if (H <= 0 || C <= 0 || ein <= 0 || H * C > (1 << 20) || ein > (1 << 20)) return fail(GNNMP_EINVAL, "gat_edge_fold: bad H/C/ein");
    if (!a_e || !W_e || !M) return fail(GNNMP_EINVAL, "gat_edge_fold: null pointer");
    const int64_t n = H * ein;
    gat_edge_fold_kernel<<<(unsigned)((n + 255) / 256), 256, 0, (hipStream_t)stream>>>(a_e, W_e, M, (int)H, (int)C, ein);
    GNNMP_LAUNCH_CHECK("gat_edge_fold_kernel");
    return GNNMP_OK;
}
extern "C" int gnnmp_gat_edge_fold_grad_f32(const float *a_e, const float *W_e, const float *dM, float *dW_e, float *da_e, int64_t H,
                                            int64_t C, int64_t ein, gnnmp_stream_t stream) {
    if (H <= 0 || C <= 0 || ein <= 0 || H * C > (1 << 20) || ein > (1 << 20)) return fail(GNNMP_EINVAL, "gat_edge_fold_grad: bad H/C/ein");
    if (!a_e || !W_e || !dM) return fail(GNNMP_EINVAL, "gat_edge_fold_grad: null pointer");
    if (!dW_e && !da_e) return GNNMP_OK;
    const int64_t n = H * C;
    gat_edge_fold_grad_kernel<<<(unsigned)((n + 255) / 256), 256, 0, (hipStream_t)stream>>>(a_e, W_e, dM, dW_e, da_e, (int)H, (int)C, ein);
    GNNMP_LAUNCH_CHECK("gat_edge_fold_grad_kernel");
    return GNNMP_OK;
}
