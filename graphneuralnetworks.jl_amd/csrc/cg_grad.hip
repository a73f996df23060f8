// cg_grad.hip — the pullback of CGConv's gated message (cg_conv, GNNlib/src/layers/conv.jl:304-333), as two passes of a row kernel.
// The forward (gnnmp_propagate_cg_f32, functor GATED = 2 of csr_reduce.h) reads three PLANAR matrices — fs_i [N][2C] (x_i's share of
// both pre-activations, biases folded in), fs_j [N][2C] (x_j's share), fs_e [E][2C] (the edge's share, optional): columns [0, C) belong
// to dense_f, columns [C, 2C) to dense_s — and computes, for edge k: j -> i and channel c,
//     f_k = fs_i[i][c]     + fs_j[j][c]     (+ fs_e[k][c])
//     s_k = fs_i[i][C + c] + fs_j[j][C + c] (+ fs_e[k][C + c])
//     m_k = sigmoid(f_k) * act(s_k),   y_i = Σ_{k into i} m_k
// Given Δ [N][C] both passes here RECOMPUTE f_k and s_k with the same additions in the same order as reduce_range<GATED = 2> and form
//     gf_k = Δ_i * act(s_k) * sigmoid'(f_k)        sigmoid'(f) = sigmoid(f) sigmoid(-f) = t r²  (t = exp(-|f|), r = 1 / (1 + t): nn_sigmoid's
//     gs_k = Δ_i * sigmoid(f_k) * act'(s_k)                                                       own two values, nothing cancels)
//     act': identity 1 | relu s > 0 (0 at 0, as gnnmp_act_grad_f32) | softplus sigmoid(s) | tanh (1 - a)(1 + a), a = tanh(s)
//   cg_grad_dst_kernel   a lane group owns destination i, walks its row of the plan: dfs_i[i] = Σ_{k into i} [gf_k | gs_k], and, when
//                        dfs_e is wanted, stores [gf_k | gs_k] at row eid (the original edge position; every edge lies in exactly one
//                        row, so every element of dfs_e is written exactly once)
//   cg_grad_src_kernel   the same walk over the TRANSPOSED plan (row j: the edges that leave j, col = the destination, eid = the original
//                        position): dfs_j[j] = Σ_{k out of j} [gf_k | gs_k]
// Whole-row walks on the shared pieces and conventions of slotwalk.h (no atomics, every output written once, a hub row by one lane group).
//
// Registers: per slot the dst pass gathers four vectors (both halves of fs_j[col] and of fs_e[eid]), the src pass five (both halves of
// fs_i[col] and of fs_e[eid], and Δ[col]).  With U = 4 slots in flight and 16-byte lanes that is 64 / 80 VGPRs of loads; the compiler's
// resource report (LABNOTES.md) shows no scratch for any instance.
#include "csr_reduce.h"
#include "launch.h"

namespace gnnmp {

struct CgGradArgs {
    PlanRows rows;               // dst pass: the plan; src pass: the transposed plan.  Whole rows (plan_rows_whole)
    RowGeom geom;
    const float *fs_i, *fs_j;    // [n][2C]
    const float *fs_e;           // [n_edges][2C], read by the HAS_E instances only
    const float *dy;             // [n][C]
    float *out;                  // dst pass: dfs_i [n][2C]; src pass: dfs_j [n][2C]
    float *dfs_e;                // dst pass, HAS_E: [n_edges][2C] or null
    int C;
};

// [gf | gs] of one edge and channel from the recomputed pre-activations and Δ
template <int ACT>
__device__ __forceinline__ void cg_edge_grad(float f, float s, float d, float &gf, float &gs) {
    const float t = hw_exp_neg_abs(f);
    const float r = __builtin_amdgcn_rcpf(1.0f + t);
    const float sig = f >= 0.0f ? r : t * r;         // nn_sigmoid(f)
    const float dsig = (t * r) * r;                   // sigmoid(f) sigmoid(-f)
    float a, da;
    if (ACT == GNNMP_ACT_RELU) {
        a = s < 0.0f ? 0.0f : s;
        da = s > 0.0f ? 1.0f : 0.0f;
    } else if (ACT == GNNMP_ACT_SOFTPLUS) {
        a = nn_softplus(s);
        da = nn_sigmoid(s);
    } else if (ACT == GNNMP_ACT_TANH) {
        a = nn_tanh(s);
        da = (1.0f - a) * (1.0f + a);
    } else {
        a = s;
        da = 1.0f;
    }
    gf = (d * a) * dsig;
    gs = (d * sig) * da;
}

template <int VEC, int U, int ACT, bool HAS_E>
__global__ void __launch_bounds__(256) cg_grad_dst_kernel(const CgGradArgs a) {
    RowLane w;
    if (!decode_row_lane<VEC>(a.rows, a.geom, a.C, w)) return;
    const int row = w.row, f0 = w.f0;
    const bool active = w.active;
    const int64_t ld = 2 * (int64_t)a.C;
    float fi[VEC], si[VEC], dv[VEC], accf[VEC], accs[VEC];
#pragma unroll
    for (int q = 0; q < VEC; ++q) accf[q] = accs[q] = 0.0f;
    load_or_zero<VEC>(active, a.fs_i + (int64_t)row * ld + f0, fi);
    load_or_zero<VEC>(active, a.fs_i + (int64_t)row * ld + a.C + f0, si);
    load_or_zero<VEC>(active, a.dy + (int64_t)row * a.C + f0, dv);
    const bool store_e = HAS_E && a.dfs_e != nullptr;
    for (uint32_t base = w.beg; base < w.end; base += w.G) {
        const Slots sl = load_slots<true, HAS_E>(a.rows.col, a.rows.eid, base, w.end, w.lig, w.G);
        for (int j = 0; j < sl.n; j += U) {
            float fj[U][VEC], sj[U][VEC], fe[HAS_E ? U : 1][VEC], se[HAS_E ? U : 1][VEC];
            int cjs[U];
            uint32_t ejs[U];
            bcast_slots<U, true, HAS_E>(sl, w.gbase, j, cjs, ejs);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (active) {      // one branch round the loads: load_or_zero per load costs <2, 4, TANH, true> a wave (LABNOTES.md)
                    Vec<VEC>::load(a.fs_j + (int64_t)cjs[u] * ld + f0, fj[u]);
                    Vec<VEC>::load(a.fs_j + (int64_t)cjs[u] * ld + a.C + f0, sj[u]);
                    if (HAS_E) {
                        Vec<VEC>::load(a.fs_e + (int64_t)ejs[u] * ld + f0, fe[HAS_E ? u : 0]);
                        Vec<VEC>::load(a.fs_e + (int64_t)ejs[u] * ld + a.C + f0, se[HAS_E ? u : 0]);
                    }
                } else {
#pragma unroll
                    for (int q = 0; q < VEC; ++q) {
                        fj[u][q] = sj[u][q] = 0.0f;
                        if (HAS_E) fe[HAS_E ? u : 0][q] = se[HAS_E ? u : 0][q] = 0.0f;
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (j + u < sl.n) {
                    float gf[VEC], gs[VEC];
#pragma unroll
                    for (int q = 0; q < VEC; ++q) {
                        float f = fi[q] + fj[u][q], s = si[q] + sj[u][q];   // as reduce_range<GATED = 2>
                        if (HAS_E) {
                            f = f + fe[HAS_E ? u : 0][q];
                            s = s + se[HAS_E ? u : 0][q];
                        }
                        cg_edge_grad<ACT>(f, s, dv[q], gf[q], gs[q]);
                        accf[q] = accf[q] + gf[q];
                        accs[q] = accs[q] + gs[q];
                    }
                    if (store_e && active) {
                        Vec<VEC>::store(a.dfs_e + (int64_t)ejs[u] * ld + f0, gf);
                        Vec<VEC>::store(a.dfs_e + (int64_t)ejs[u] * ld + a.C + f0, gs);
                    }
                }
            }
        }
    }
    if (active) {
        Vec<VEC>::store(a.out + (int64_t)row * ld + f0, accf);
        Vec<VEC>::store(a.out + (int64_t)row * ld + a.C + f0, accs);
    }
}

template <int VEC, int U, int ACT, bool HAS_E>
__global__ void __launch_bounds__(256) cg_grad_src_kernel(const CgGradArgs a) {
    RowLane w;
    if (!decode_row_lane<VEC>(a.rows, a.geom, a.C, w)) return;
    const int row = w.row, f0 = w.f0;
    const bool active = w.active;
    const int64_t ld = 2 * (int64_t)a.C;
    float fj[VEC], sj[VEC], accf[VEC], accs[VEC];
#pragma unroll
    for (int q = 0; q < VEC; ++q) accf[q] = accs[q] = 0.0f;
    load_or_zero<VEC>(active, a.fs_j + (int64_t)row * ld + f0, fj);      // this source's share of both pre-activations
    load_or_zero<VEC>(active, a.fs_j + (int64_t)row * ld + a.C + f0, sj);
    for (uint32_t base = w.beg; base < w.end; base += w.G) {
        const Slots sl = load_slots<true, HAS_E>(a.rows.col, a.rows.eid, base, w.end, w.lig, w.G);      // col: the destination of the edge
        for (int j = 0; j < sl.n; j += U) {
            float fi[U][VEC], si[U][VEC], dv[U][VEC], fe[HAS_E ? U : 1][VEC], se[HAS_E ? U : 1][VEC];
            int cjs[U];
            uint32_t ejs[U];
            bcast_slots<U, true, HAS_E>(sl, w.gbase, j, cjs, ejs);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t ci = cjs[u];
                if (active) {
                    Vec<VEC>::load(a.fs_i + ci * ld + f0, fi[u]);
                    Vec<VEC>::load(a.fs_i + ci * ld + a.C + f0, si[u]);
                    Vec<VEC>::load(a.dy + ci * a.C + f0, dv[u]);
                    if (HAS_E) {
                        Vec<VEC>::load(a.fs_e + (int64_t)ejs[u] * ld + f0, fe[HAS_E ? u : 0]);
                        Vec<VEC>::load(a.fs_e + (int64_t)ejs[u] * ld + a.C + f0, se[HAS_E ? u : 0]);
                    }
                } else {
#pragma unroll
                    for (int q = 0; q < VEC; ++q) {
                        fi[u][q] = si[u][q] = dv[u][q] = 0.0f;
                        if (HAS_E) fe[HAS_E ? u : 0][q] = se[HAS_E ? u : 0][q] = 0.0f;
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (j + u < sl.n) {
#pragma unroll
                    for (int q = 0; q < VEC; ++q) {
                        float f = fi[u][q] + fj[q], s = si[u][q] + sj[q];   // fs_i first, as the forward adds them
                        if (HAS_E) {
                            f = f + fe[HAS_E ? u : 0][q];
                            s = s + se[HAS_E ? u : 0][q];
                        }
                        float gf, gs;
                        cg_edge_grad<ACT>(f, s, dv[u][q], gf, gs);
                        accf[q] = accf[q] + gf;
                        accs[q] = accs[q] + gs;
                    }
                }
            }
        }
    }
    if (active) {
        Vec<VEC>::store(a.out + (int64_t)row * ld + f0, accf);
        Vec<VEC>::store(a.out + (int64_t)row * ld + a.C + f0, accs);
    }
}

}  // namespace gnnmp

using namespace gnnmp;

extern "C" int gnnmp_cg_conv_grad_f32(const gnnmp_graph_t *plan, const gnnmp_graph_t *plan_t, const gnnmp_cg_conv_grad_t *job, int64_t C,
                                      gnnmp_stream_t stream) {
    if (!plan) return fail(GNNMP_EINVAL, "cg_conv_grad: null plan");
    if (!plan_t) return fail(GNNMP_EINVAL, "cg_conv_grad: null plan_t");
    if (!job) return fail(GNNMP_EINVAL, "cg_conv_grad: null job");
    if (!job->fs_i) return fail(GNNMP_EINVAL, "cg_conv_grad: null fs_i");
    if (!job->fs_j) return fail(GNNMP_EINVAL, "cg_conv_grad: null fs_j");
    if (!job->dy) return fail(GNNMP_EINVAL, "cg_conv_grad: null dy");
    if (!job->dfs_i) return fail(GNNMP_EINVAL, "cg_conv_grad: null dfs_i");
    if (!job->dfs_j) return fail(GNNMP_EINVAL, "cg_conv_grad: null dfs_j");
    if (job->dfs_e && !job->fs_e) return fail(GNNMP_EINVAL, "cg_conv_grad: dfs_e without fs_e");
    if (C < 1 || C > (1 << 19)) return fail(GNNMP_EINVAL, "cg_conv_grad: bad C %lld", (long long)C);
    if (job->act < GNNMP_ACT_IDENTITY || job->act > GNNMP_ACT_TANH) return fail(GNNMP_EINVAL, "cg_conv_grad: bad act %d", job->act);
    GNNMP_TRY(check_edge_plan("cg_conv_grad", plan, plan_t, true, "fs_e has no row for them"));
    if (plan->n_dst == 0) return GNNMP_OK;
    CgGradArgs a = {};
    a.rows = plan_rows_whole(plan);
    a.fs_i = job->fs_i;
    a.fs_j = job->fs_j;
    a.fs_e = job->fs_e;
    a.dy = job->dy;
    a.out = job->dfs_i;
    a.dfs_e = job->dfs_e;
    a.C = (int)C;
    dim3 grid;
    const int vec = row_walk_geom("cg_conv_grad", a.rows, C, 0, {job->fs_i, job->fs_j, job->fs_e, job->dy, job->dfs_i, job->dfs_j, job->dfs_e},
                                  a.geom, grid);
    if (vec < 0) return vec;
    const bool has_e = job->fs_e != nullptr;
    auto launch = [&](bool src) {      // the dst pass over a.rows = the plan, then the src pass over the transposed plan
        with_vec(vec, [&](auto V) {
            with_act<GNNMP_ACT_TANH>(job->act, [&](auto A) {
                constexpr int VEC = decltype(V)::value, ACT = decltype(A)::value;
                if (src && has_e)
                    cg_grad_src_kernel<VEC, 4, ACT, true><<<grid, 256, 0, (hipStream_t)stream>>>(a);
                else if (src)
                    cg_grad_src_kernel<VEC, 4, ACT, false><<<grid, 256, 0, (hipStream_t)stream>>>(a);
                else if (has_e)
                    cg_grad_dst_kernel<VEC, 4, ACT, true><<<grid, 256, 0, (hipStream_t)stream>>>(a);
                else
                    cg_grad_dst_kernel<VEC, 4, ACT, false><<<grid, 256, 0, (hipStream_t)stream>>>(a);
            });
        });
    };
    launch(false);
    GNNMP_LAUNCH_CHECK("cg_grad_dst_kernel");
    a.rows = plan_rows_whole(plan_t);      // the same heights: the same geometry and grid
    a.out = job->dfs_j;
    a.dfs_e = nullptr;
    launch(true);
    GNNMP_LAUNCH_CHECK("cg_grad_src_kernel");
    return GNNMP_OK;
}
