// gmm.hip — GMMConv (gmm_conv, GNNlib/src/layers/conv.jl:372-401) without its [E][K C] and [N][K C] arrays: the fused forward, its pullback
// and the pullback of the mixture weights.  Edge e: j -> i, kernel k < K, channel c < C; w [E][K] are the mixture weights
// (gnnmp_gmm_weights_f32 with C = 1), xk = x dense_x_weight' [N][K C] with kernel k's block at k C (include/gnnmp.h states the arithmetic):
//   gmm_conv_kernel        a lane group owns destination i; a lane holds K accumulators for each of its VEC channels.  For every edge into
//                          i, in edge order: acc[k][c] = acc[k][c] + w[e][k] * xk[j][k C + c] — A MULTIPLY AND AN ADD, the product rounded
//                          (the library is built with -ffp-contract=off).  Then m_k = acc[k] / deg_i (deg_i = 0: the zero it is),
//                          z = ((m_0 + m_1) + ... + m_{K-1}) / K (+ bias), y = act(z) by bias_act_apply, the device function of
//                          gnnmp_bias_act_f32.  The K weights of an edge are read once per edge, at the edge's original position.
//   gmm_conv_grad_kernel   a lane group owns source j (a row of the TRANSPOSED plan) and holds xk[j] in registers.  For every edge e: j -> i
//                          that leaves j, in edge order, with q_i = 1 / (K max(deg_i, 1)) (deg_i from the plan's rowptr) and
//                          t[c] = q_i * dz[i][c]:   dxk[j][k C + c] += w[e][k] * t[c]      dw[e][k] = Σ_c xk[j][k C + c] * t[c]
//                          The lane sums its own channels in ascending order, the G lane partials go through a butterfly
//                          (p[l] + p[l ^ m], m = G/2 .. 1), and — only when C needs more than one tile of G VEC channels — the tiles are
//                          walked one after the other by the SAME lane group and added to dw[e][k] in tile order by the lane that wrote it.
//   gmm_de_kernel          one thread an edge: g_k = dw[e][k] * w[e][k], de[e][d] = Σ_k (g_k (e[e][d] − mu[k][d])) * sinv[k][d]², k ascending
//   gmm_wfold_kernel       GNNMP_GMM_PARTS blocks; block b folds the edges [b L, min(E, (b + 1) L)), L = ceil(E / GNNMP_GMM_PARTS), into
//                          part[b][0][k][d] (dmu) and part[b][1][k][d] (dsinv): a wave takes the elements (k, d) = wave, wave + 4, ...; lane
//                          l folds the slice's edges l, l + 64, ... sequentially from 0, then a 64-lane butterfly.  Every element of part
//                          is written (an empty slice: zeros).
//   gmm_wfinal_kernel      one block: dmu / dsinv [k][d] = part[0] + part[1] + ... in index order, from 0.
// No scratch but the caller's `part`.  The row kernels are whole-row walks on the shared pieces and conventions of slotwalk.h (no atomics,
// every output written once, a hub row by one lane group).
//
// Registers: the accumulators (and, in the pullback, xk[j]) live in registers, so the row kernels are instantiated for the capacities
// KC = 1, 2, 3, 4, 8, 16 (the smallest one that holds K; kernels beyond K load nothing and add nothing).  DESIGN.md §3 has the compiler's
// resource report: no instance uses scratch.
#include "csr_reduce.h"
#include "launch.h"

namespace gnnmp {

// edges in flight per lane group: U K row loads are outstanding
template <int KC>
constexpr int gmm_u() {
    return KC == 1 ? 4 : (KC <= 3 ? 2 : 1);
}

// ---- forward ----------------------------------------------------------------------------------------------------------------------
struct GmmConvArgs {
    PlanRows rows;      // whole rows (plan_rows_whole)
    RowGeom geom;
    const float *w;     // [n_edges][K]
    const float *xk;    // [n][K C]
    const float *bias;  // [C] or null
    float *y, *z;       // [n][C]; z or null
    int K, C, act;
};

template <int VEC, int KC>
__global__ void __launch_bounds__(256) gmm_conv_kernel(const GmmConvArgs a) {
    constexpr int U = gmm_u<KC>();
    RowLane w;
    if (!decode_row_lane<VEC>(a.rows, a.geom, a.C, w)) return;
    const int row = w.row, f0 = w.f0;
    const bool active = w.active;
    const uint32_t beg = w.beg, end = w.end;
    const int64_t ld = (int64_t)a.K * a.C;
    float acc[KC][VEC];
#pragma unroll
    for (int k = 0; k < KC; ++k) {
#pragma unroll
        for (int q = 0; q < VEC; ++q) acc[k][q] = 0.0f;
    }
    for (uint32_t base = beg; base < end; base += w.G) {
        const Slots sl = load_slots<true, true>(a.rows.col, a.rows.eid, base, end, w.lig, w.G);
        for (int j = 0; j < sl.n; j += U) {
            float v[U][KC][VEC], wk[U][KC];
            int cjs[U];
            uint32_t ejs[U];
            bcast_slots<U, true, true>(sl, w.gbase, j, cjs, ejs);
#pragma unroll
            for (int u = 0; u < U; ++u) {
#pragma unroll
                for (int k = 0; k < KC; ++k) {
                    if (k < a.K) {
                        wk[u][k] = a.w[(int64_t)ejs[u] * a.K + k];
                        load_or_zero<VEC>(active, a.xk + (int64_t)cjs[u] * ld + (int64_t)k * a.C + f0, v[u][k]);
                    } else {
                        wk[u][k] = 0.0f;
#pragma unroll
                        for (int q = 0; q < VEC; ++q) v[u][k][q] = 0.0f;
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (j + u < sl.n) {
#pragma unroll
                    for (int k = 0; k < KC; ++k) {
#pragma unroll
                        for (int q = 0; q < VEC; ++q) acc[k][q] = acc[k][q] + wk[u][k] * v[u][k][q];   // product rounded, then added
                    }
                }
            }
        }
    }
    if (!active) return;
    const uint32_t deg = end - beg;
    const float fdeg = (float)deg, fk = (float)a.K;
    float s[VEC];
#pragma unroll
    for (int q = 0; q < VEC; ++q) s[q] = deg ? acc[0][q] / fdeg : acc[0][q];
#pragma unroll
    for (int k = 1; k < KC; ++k) {
        if (k < a.K) {
#pragma unroll
            for (int q = 0; q < VEC; ++q) s[q] = s[q] + (deg ? acc[k][q] / fdeg : acc[k][q]);
        }
    }
#pragma unroll
    for (int q = 0; q < VEC; ++q) s[q] = s[q] / fk;
    if (a.bias) {
        float b[VEC];
        Vec<VEC>::load(a.bias + f0, b);
#pragma unroll
        for (int q = 0; q < VEC; ++q) s[q] = s[q] + b[q];
    }
    if (a.z) Vec<VEC>::store(a.z + (int64_t)row * a.C + f0, s);
#pragma unroll
    for (int q = 0; q < VEC; ++q) s[q] = bias_act_apply(s[q], a.act);
    Vec<VEC>::store(a.y + (int64_t)row * a.C + f0, s);
}

// ---- pullback of the row step -----------------------------------------------------------------------------------------------------------
struct GmmGradArgs {
    PlanRows rows;             // the TRANSPOSED plan, whole rows: row j lists the edges that leave j, col = the destination
    const uint32_t *rowptr;    // the plan's own rowptr: the in-degree of a destination
    RowGeom geom;
    const float *w, *xk, *dz;
    float *dxk, *dw;
    int K, C, tiles;
};

template <int VEC, int KC, bool WANT_DXK, bool WANT_DW>
__global__ void __launch_bounds__(256) gmm_conv_grad_kernel(const GmmGradArgs a) {
    constexpr int U = 2;
    VRow w;      // no RowLane: the lane group walks the feature tiles itself
    if (!decode_vrow<VROW_WHOLE>(a.rows, a.geom, blockIdx.x, w)) return;
    const int row = w.row, lig = w.lig, G = w.G;
    const int64_t ld = (int64_t)a.K * a.C;
    const float fk = (float)a.K;
    for (int tt = 0; tt < a.tiles; ++tt) {      // one tile unless C > 64 VEC: dw's sum over channels stays inside this lane group
        const int f0 = (tt * G + lig) * VEC;
        const bool active = f0 < a.C;
        float xr[WANT_DW ? KC : 1][VEC], acc[WANT_DXK ? KC : 1][VEC];
#pragma unroll
        for (int k = 0; k < KC; ++k) {
#pragma unroll
            for (int q = 0; q < VEC; ++q) {
                if (WANT_DW) xr[WANT_DW ? k : 0][q] = 0.0f;
                if (WANT_DXK) acc[WANT_DXK ? k : 0][q] = 0.0f;
            }
            if (WANT_DW && active && k < a.K) Vec<VEC>::load(a.xk + (int64_t)row * ld + (int64_t)k * a.C + f0, xr[WANT_DW ? k : 0]);
        }
        for (uint32_t base = w.beg; base < w.end; base += G) {
            const Slots sl = load_slots<true, true>(a.rows.col, a.rows.eid, base, w.end, lig, G);      // col: the destination of the edge
            float qv = 0.0f;
            if (base + lig < w.end) {
                const uint32_t deg = a.rowptr[sl.c + 1] - a.rowptr[sl.c];      // >= 1: this edge enters c
                qv = 1.0f / (fk * (float)max(deg, 1u));
            }
            for (int j = 0; j < sl.n; j += U) {
                float d[U][VEC], wk[U][KC], qs[U];
                uint32_t ejs[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {      // the broadcast stays here, slot by slot with its loads: bcast_slots ahead of the
                    const int jj = min(j + u, sl.n - 1);      // loop costs <1, 16, true, true> and <2, 4, true, true> a wave (LABNOTES.md)
                    const int cj = __shfl(sl.c, w.gbase + jj, 64);
                    ejs[u] = (uint32_t)__shfl((int)sl.ev, w.gbase + jj, 64);
                    qs[u] = __shfl(qv, w.gbase + jj, 64);
                    load_or_zero<VEC>(active, a.dz + (int64_t)cj * a.C + f0, d[u]);
#pragma unroll
                    for (int k = 0; k < KC; ++k) wk[u][k] = (WANT_DXK && k < a.K) ? a.w[(int64_t)ejs[u] * a.K + k] : 0.0f;     // dw reads no w
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    if (j + u < sl.n) {      // uniform over the lane group: every lane of it takes part in the butterfly
                        float t[VEC];
#pragma unroll
                        for (int q = 0; q < VEC; ++q) t[q] = qs[u] * d[u][q];
                        if (WANT_DXK) {
#pragma unroll
                            for (int k = 0; k < KC; ++k) {
#pragma unroll
                                for (int q = 0; q < VEC; ++q) acc[WANT_DXK ? k : 0][q] = acc[WANT_DXK ? k : 0][q] + wk[u][k] * t[q];
                            }
                        }
                        if (WANT_DW) {
                            float pk[KC];
#pragma unroll
                            for (int k = 0; k < KC; ++k) {
                                pk[k] = 0.0f;
#pragma unroll
                                for (int q = 0; q < VEC; ++q) pk[k] = pk[k] + xr[WANT_DW ? k : 0][q] * t[q];
                            }
                            group_sum<KC>(pk, G);
                            if (lig == 0) {
                                float *o = a.dw + (int64_t)ejs[u] * a.K;
#pragma unroll
                                for (int k = 0; k < KC; ++k) {
                                    if (k < a.K) o[k] = tt == 0 ? pk[k] : o[k] + pk[k];     // a later tile: this lane's own earlier store
                                }
                            }
                        }
                    }
                }
            }
        }
        if (WANT_DXK && active) {
#pragma unroll
            for (int k = 0; k < KC; ++k) {
                if (k < a.K) Vec<VEC>::store(a.dxk + (int64_t)row * ld + (int64_t)k * a.C + f0, acc[WANT_DXK ? k : 0]);
            }
        }
    }
}

// ---- pullback of the mixture weights ------------------------------------------------------------------------------------------------------
struct GmmWgradArgs {
    const float *e, *mu, *sinv, *w, *dw;
    float *de, *dmu, *dsinv, *part;
    int64_t E;
    int ein, K;
};

__global__ void __launch_bounds__(256) gmm_de_kernel(const GmmWgradArgs a) {
    const int64_t ed = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (ed >= a.E) return;
    float g[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) g[k] = k < a.K ? a.dw[ed * a.K + k] * a.w[ed * a.K + k] : 0.0f;
    for (int d = 0; d < a.ein; ++d) {
        const float ev = a.e[ed * a.ein + d];
        float s = 0.0f;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            if (k < a.K) {
                const float diff = ev - a.mu[k * a.ein + d], si = a.sinv[k * a.ein + d];
                s = s + (g[k] * diff) * (si * si);
            }
        }
        a.de[ed * a.ein + d] = s;
    }
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) v = v + __shfl_xor(v, m, 64);
    return v;
}

__global__ void __launch_bounds__(256) gmm_wfold_kernel(const GmmWgradArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t L = (a.E + GNNMP_GMM_PARTS - 1) / GNNMP_GMM_PARTS;
    const int64_t beg = min(a.E, (int64_t)blockIdx.x * L), end = min(a.E, beg + L);
    const int M = a.K * a.ein;
    float *part = a.part + (int64_t)blockIdx.x * 2 * M;
    for (int m = wave; m < M; m += 4) {      // uniform over the wave
        const int k = m / a.ein, d = m - k * a.ein;
        const float muv = a.mu[m], si = a.sinv[m];
        float am = 0.0f, as = 0.0f;
        for (int64_t ed = beg + lane; ed < end; ed += 64) {
            const float g = a.dw[ed * a.K + k] * a.w[ed * a.K + k];
            const float diff = a.e[ed * a.ein + d] - muv;
            am = am - (g * diff) * (si * si);
            as = as + (g * (diff * diff)) * si;
        }
        am = wave_sum(am);
        as = wave_sum(as);
        if (lane == 0) {
            part[m] = am;
            part[M + m] = as;
        }
    }
}

__global__ void __launch_bounds__(256) gmm_wfinal_kernel(const GmmWgradArgs a) {
    const int M = a.K * a.ein;
    for (int i = threadIdx.x; i < 2 * M; i += 256) {
        float s = 0.0f;
        for (int b = 0; b < GNNMP_GMM_PARTS; ++b) s = s + a.part[(int64_t)b * 2 * M + i];
        if (i < M)
            a.dmu[i] = s;
        else
            a.dsinv[i - M] = s;
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------------
// the register capacity that holds K kernels
template <class F>
static void with_kc(int K, F &&f) {
    if (K <= 1) return f(int_c<1>{});
    if (K == 2) return f(int_c<2>{});
    if (K == 3) return f(int_c<3>{});
    if (K == 4) return f(int_c<4>{});
    if (K <= 8) return f(int_c<8>{});
    return f(int_c<16>{});
}

static int gmm_check_sizes(const char *who, int64_t K, int64_t C) {
    if (K < 1 || K > 16) return fail(GNNMP_EINVAL, "%s: bad K %lld", who, (long long)K);
    if (C < 1 || C > (1 << 19) || K * C > (1 << 20)) return fail(GNNMP_EINVAL, "%s: bad C %lld", who, (long long)C);
    return GNNMP_OK;
}

}  // namespace gnnmp

using namespace gnnmp;

extern "C" int gnnmp_gmm_conv_f32(const gnnmp_graph_t *plan, const gnnmp_gmm_conv_t *job, int64_t K, int64_t C, gnnmp_stream_t stream) {
    if (!plan) return fail(GNNMP_EINVAL, "gmm_conv: null plan");
    if (!job) return fail(GNNMP_EINVAL, "gmm_conv: null job");
    if (!job->w && plan->n_total > 0) return fail(GNNMP_EINVAL, "gmm_conv: null w");      // no edge: no entry of w is read
    if (!job->xk) return fail(GNNMP_EINVAL, "gmm_conv: null xk");
    if (!job->y) return fail(GNNMP_EINVAL, "gmm_conv: null y");
    GNNMP_TRY(gmm_check_sizes("gmm_conv", K, C));
    if (job->act < GNNMP_ACT_IDENTITY || job->act > GNNMP_ACT_SWISH) return fail(GNNMP_EINVAL, "gmm_conv: bad act %d", job->act);
    GNNMP_TRY(check_edge_plan("gmm_conv", plan, nullptr, true, "w has no row for them"));
    if (plan->n_dst == 0) return GNNMP_OK;
    GmmConvArgs a = {};
    a.rows = plan_rows_whole(plan);
    a.w = job->w;
    a.xk = job->xk;
    a.bias = job->bias;
    a.y = job->y;
    a.z = job->z;
    a.K = (int)K;
    a.C = (int)C;
    a.act = job->act;
    dim3 grid;
    const int vec = row_walk_geom("gmm_conv", a.rows, C, 0, {job->xk, job->bias, job->y, job->z}, a.geom, grid);
    if (vec < 0) return vec;
    with_vec(vec, [&](auto V) {
        with_kc(a.K, [&](auto KC) { gmm_conv_kernel<decltype(V)::value, decltype(KC)::value><<<grid, 256, 0, (hipStream_t)stream>>>(a); });
    });
    GNNMP_LAUNCH_CHECK("gmm_conv_kernel");
    return GNNMP_OK;
}

extern "C" int gnnmp_gmm_conv_grad_f32(const gnnmp_graph_t *plan, const gnnmp_graph_t *plan_t, const gnnmp_gmm_conv_grad_t *job, int64_t K,
                                       int64_t C, gnnmp_stream_t stream) {
    if (!plan) return fail(GNNMP_EINVAL, "gmm_conv_grad: null plan");
    if (!plan_t) return fail(GNNMP_EINVAL, "gmm_conv_grad: null plan_t");
    if (!job) return fail(GNNMP_EINVAL, "gmm_conv_grad: null job");
    if (!job->dxk && !job->dw) return fail(GNNMP_EINVAL, "gmm_conv_grad: dxk and dw are both null");
    if (!job->dz) return fail(GNNMP_EINVAL, "gmm_conv_grad: null dz");
    if (job->dxk && !job->w && plan->n_total > 0) return fail(GNNMP_EINVAL, "gmm_conv_grad: dxk without w");      // no edge: not read
    if (job->dw && !job->xk) return fail(GNNMP_EINVAL, "gmm_conv_grad: dw without xk");
    GNNMP_TRY(gmm_check_sizes("gmm_conv_grad", K, C));
    GNNMP_TRY(check_edge_plan("gmm_conv_grad", plan, plan_t, true, "w has no row for them"));
    if (plan->n_dst == 0) return GNNMP_OK;
    const bool want_dxk = job->dxk != nullptr, want_dw = job->dw != nullptr;
    GmmGradArgs a = {};
    a.rows = plan_rows_whole(plan_t);
    a.rowptr = plan->rowptr;
    a.w = job->w;
    a.xk = job->xk;
    a.dz = job->dz;
    a.dxk = job->dxk;
    a.dw = job->dw;
    a.K = (int)K;
    a.C = (int)C;
    dim3 grid;      // one block per row group: the lane group walks the feature tiles itself
    const int vec = row_walk_geom("gmm_conv_grad", a.rows, C, 1, {want_dw ? job->xk : nullptr, job->dz, job->dxk}, a.geom, grid);
    if (vec < 0) return vec;
    a.tiles = feature_tiles(C, vec, a.geom.log2g);
    with_vec(vec, [&](auto V) {
        with_kc(a.K, [&](auto KC) {
            constexpr int VEC = decltype(V)::value, KCV = decltype(KC)::value;
            if (want_dxk && want_dw)
                gmm_conv_grad_kernel<VEC, KCV, true, true><<<grid, 256, 0, (hipStream_t)stream>>>(a);
            else if (want_dxk)
                gmm_conv_grad_kernel<VEC, KCV, true, false><<<grid, 256, 0, (hipStream_t)stream>>>(a);
            else
                gmm_conv_grad_kernel<VEC, KCV, false, true><<<grid, 256, 0, (hipStream_t)stream>>>(a);
        });
    });
    GNNMP_LAUNCH_CHECK("gmm_conv_grad_kernel");
    return GNNMP_OK;
}

extern "C" int gnnmp_gmm_weights_grad_f32(const gnnmp_gmm_weights_grad_t *job, int64_t E, int64_t ein, int64_t K, gnnmp_stream_t stream) {
    if (!job) return fail(GNNMP_EINVAL, "gmm_weights_grad: null job");
    if (E < 0) return fail(GNNMP_EINVAL, "gmm_weights_grad: negative E");
    if (ein < 1 || ein > 64) return fail(GNNMP_EINVAL, "gmm_weights_grad: bad ein %lld", (long long)ein);
    if (K < 1 || K > 16) return fail(GNNMP_EINVAL, "gmm_weights_grad: bad K %lld", (long long)K);
    if (!job->de && !job->dmu && !job->dsinv) return fail(GNNMP_EINVAL, "gmm_weights_grad: de, dmu and dsinv are all null");
    if ((job->dmu == nullptr) != (job->dsinv == nullptr)) return fail(GNNMP_EINVAL, "gmm_weights_grad: dmu and dsinv come together");
    if (job->dmu && !job->part) return fail(GNNMP_EINVAL, "gmm_weights_grad: dmu without part");
    if (E == 0) return GNNMP_OK;
    if (!job->e) return fail(GNNMP_EINVAL, "gmm_weights_grad: null e");
    if (!job->mu) return fail(GNNMP_EINVAL, "gmm_weights_grad: null mu");
    if (!job->sinv) return fail(GNNMP_EINVAL, "gmm_weights_grad: null sinv");
    if (!job->w) return fail(GNNMP_EINVAL, "gmm_weights_grad: null w");
    if (!job->dw) return fail(GNNMP_EINVAL, "gmm_weights_grad: null dw");
    const int64_t blocks = (E + 255) / 256;
    if (blocks >= INT32_MAX) return fail(GNNMP_EUNSUPPORTED, "gmm_weights_grad: too many edge blocks");
    GmmWgradArgs a = {};
    a.e = job->e;
    a.mu = job->mu;
    a.sinv = job->sinv;
    a.w = job->w;
    a.dw = job->dw;
    a.de = job->de;
    a.dmu = job->dmu;
    a.dsinv = job->dsinv;
    a.part = job->part;
    a.E = E;
    a.ein = (int)ein;
    a.K = (int)K;
    if (job->de) {
        gmm_de_kernel<<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(a);
        GNNMP_LAUNCH_CHECK("gmm_de_kernel");
    }
    if (job->dmu) {
        gmm_wfold_kernel<<<GNNMP_GMM_PARTS, 256, 0, (hipStream_t)stream>>>(a);
        GNNMP_LAUNCH_CHECK("gmm_wfold_kernel");
        gmm_wfinal_kernel<<<1, 256, 0, (hipStream_t)stream>>>(a);
        GNNMP_LAUNCH_CHECK("gmm_wfinal_kernel");
    }
    return GNNMP_OK;
}
