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
// No atomics, no plan-owned scratch, every output element written exactly once (rows without in-edges and rows without out-edges
// included: zeros).  Both kernels walk every row WHOLE, in edge order, whatever its length (PlanRows with n_chunks = 0, VROW_WHOLE),
// as edge_conv.hip does: every sum has the bits of the sequential fold, two calls give equal bits, and A HUB ROW IS WALKED BY ONE LANE
// GROUP: correct, slow.  Chunked hub rows are a later change.
//
// Registers: per slot the dst pass gathers four vectors (both halves of fs_j[col] and of fs_e[eid]), the src pass five (both halves of
// fs_i[col] and of fs_e[eid], and Δ[col]).  With U = 4 slots in flight and 16-byte lanes that is 64 / 80 VGPRs of loads; the compiler's
// resource report (LABNOTES.md) shows no scratch for any instance.
#include "csr_reduce.h"

namespace gnnmp {

struct CgGradArgs {
    PlanRows rows;               // dst pass: the plan; src pass: the transposed plan.  n_chunks = 0 (rows are walked whole)
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
    VRow vr;
    if (!decode_vrow<VROW_WHOLE>(a.rows, a.geom, blockIdx.x, vr)) return;
    const int row = vr.row, lig = vr.lig, gbase = vr.gbase, G = vr.G;
    const uint32_t beg = vr.beg, end = vr.end;
    const int f0 = ((int)blockIdx.y * G + lig) * VEC;
    const bool active = f0 < a.C;      // inactive lanes of the last feature tile load nothing and store nothing
    const int64_t ld = 2 * (int64_t)a.C;
    float fi[VEC], si[VEC], dv[VEC], accf[VEC], accs[VEC];
#pragma unroll
    for (int q = 0; q < VEC; ++q) fi[q] = si[q] = dv[q] = accf[q] = accs[q] = 0.0f;
    if (active) {
        Vec<VEC>::load(a.fs_i + (int64_t)row * ld + f0, fi);
        Vec<VEC>::load(a.fs_i + (int64_t)row * ld + a.C + f0, si);
        Vec<VEC>::load(a.dy + (int64_t)row * a.C + f0, dv);
    }
    const bool store_e = HAS_E && a.dfs_e != nullptr;
    for (uint32_t base = beg; base < end; base += G) {   // slots are unsigned 32-bit (rowwalk.h)
        const uint32_t p = base + lig;
        int c = 0;
        uint32_t ev = 0;
        if (p < end) {
            c = a.rows.col[p];
            if (HAS_E) ev = (uint32_t)a.rows.eid[p];    // < n_edges: the export refuses a plan with self loops of its own
        }
        const int n = (int)min((uint32_t)G, end - base);
        for (int j = 0; j < n; j += U) {
            float fj[U][VEC], sj[U][VEC], fe[HAS_E ? U : 1][VEC], se[HAS_E ? U : 1][VEC];
            int cjs[U];
            uint32_t ejs[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int jj = min(j + u, n - 1);
                cjs[u] = __shfl(c, gbase + jj, 64);
                ejs[u] = HAS_E ? (uint32_t)__shfl((int)ev, gbase + jj, 64) : 0u;
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (active) {   // clamped, unconditional within the lane's activity (edge_conv.hip)
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
                if (j + u < n) {
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
    VRow vr;
    if (!decode_vrow<VROW_WHOLE>(a.rows, a.geom, blockIdx.x, vr)) return;
    const int row = vr.row, lig = vr.lig, gbase = vr.gbase, G = vr.G;
    const uint32_t beg = vr.beg, end = vr.end;
    const int f0 = ((int)blockIdx.y * G + lig) * VEC;
    const bool active = f0 < a.C;
    const int64_t ld = 2 * (int64_t)a.C;
    float fj[VEC], sj[VEC], accf[VEC], accs[VEC];
#pragma unroll
    for (int q = 0; q < VEC; ++q) fj[q] = sj[q] = accf[q] = accs[q] = 0.0f;
    if (active) {   // this source's share of both pre-activations
        Vec<VEC>::load(a.fs_j + (int64_t)row * ld + f0, fj);
        Vec<VEC>::load(a.fs_j + (int64_t)row * ld + a.C + f0, sj);
    }
    for (uint32_t base = beg; base < end; base += G) {
        const uint32_t p = base + lig;
        int c = 0;
        uint32_t ev = 0;
        if (p < end) {
            c = a.rows.col[p];                           // the destination of the edge
            if (HAS_E) ev = (uint32_t)a.rows.eid[p];
        }
        const int n = (int)min((uint32_t)G, end - base);
        for (int j = 0; j < n; j += U) {
            float fi[U][VEC], si[U][VEC], dv[U][VEC], fe[HAS_E ? U : 1][VEC], se[HAS_E ? U : 1][VEC];
            int cjs[U];
            uint32_t ejs[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int jj = min(j + u, n - 1);
                cjs[u] = __shfl(c, gbase + jj, 64);
                ejs[u] = HAS_E ? (uint32_t)__shfl((int)ev, gbase + jj, 64) : 0u;
            }
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
                if (j + u < n) {
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

static PlanRows cg_whole_rows(const gnnmp_graph_t *plan) {
    PlanRows r = plan_rows(plan);
    r.n_chunks = 0;     // no chunk virtual rows: VROW_WHOLE walks the long rows themselves
    r.n_long = 0;
    return r;
}

// the vector width every array of the call admits — column C inside a row included — and the row walk's geometry for it
static int cg_grad_geom(CgGradArgs &a, const gnnmp_cg_conv_grad_t *job, dim3 &grid) {
    uintptr_t align = 0;
    const float *const ptrs[] = {job->fs_i, job->fs_j, job->fs_e, job->dy, job->dfs_i, job->dfs_j, job->dfs_e};
    for (const float *p : ptrs) {
        if (p) align |= reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(p + a.C);
    }
    const int vec = pick_vec(a.C, reinterpret_cast<const void *>(align), nullptr);
    a.geom = RowGeom{pick_log2g((a.C + vec - 1) / vec), 4, 0, 0};
    if (row_blocks(a.rows, a.geom) >= INT32_MAX) return fail(GNNMP_EUNSUPPORTED, "cg_conv_grad: too many row blocks");
    grid = row_grid(a.rows, a.geom, feature_tiles(a.C, vec, a.geom.log2g));
    return vec;
}

template <class F>
static void with_cg_act(int act, F &&f) {
    switch (act) {
        case GNNMP_ACT_RELU: return f(int_c<GNNMP_ACT_RELU>{});
        case GNNMP_ACT_SOFTPLUS: return f(int_c<GNNMP_ACT_SOFTPLUS>{});
        case GNNMP_ACT_TANH: return f(int_c<GNNMP_ACT_TANH>{});
        default: return f(int_c<GNNMP_ACT_IDENTITY>{});
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
    if (plan->n_src != plan->n_dst)
        return fail(GNNMP_EINVAL, "cg_conv_grad: the plan is not square (%lld sources, %lld destinations)", (long long)plan->n_src,
                    (long long)plan->n_dst);
    if (plan_t->n_dst != plan->n_dst || plan_t->n_src != plan->n_src)
        return fail(GNNMP_EINVAL, "cg_conv_grad: the transposed plan has %lld rows, the plan %lld", (long long)plan_t->n_dst, (long long)plan->n_dst);
    if (plan_t->n_edges != plan->n_edges || plan_t->n_total != plan->n_total)
        return fail(GNNMP_EINVAL, "cg_conv_grad: the transposed plan has %lld edges, the plan %lld", (long long)plan_t->n_total, (long long)plan->n_total);
    if (plan->n_total != plan->n_edges)
        return fail(GNNMP_EINVAL, "cg_conv_grad: the plan was built with self loops (%lld slots, %lld edges): fs_e has no row for them",
                    (long long)plan->n_total, (long long)plan->n_edges);
    if (plan->n_dst == 0) return GNNMP_OK;
    CgGradArgs a = {};
    a.rows = cg_whole_rows(plan);
    a.fs_i = job->fs_i;
    a.fs_j = job->fs_j;
    a.fs_e = job->fs_e;
    a.dy = job->dy;
    a.out = job->dfs_i;
    a.dfs_e = job->dfs_e;
    a.C = (int)C;
    dim3 grid;
    const int vec = cg_grad_geom(a, job, grid);
    if (vec < 0) return vec;
    const bool has_e = job->fs_e != nullptr;
    with_vec(vec, [&](auto V) {
        with_cg_act(job->act, [&](auto A) {
            if (has_e)
                cg_grad_dst_kernel<decltype(V)::value, 4, decltype(A)::value, true><<<grid, 256, 0, (hipStream_t)stream>>>(a);
            else
                cg_grad_dst_kernel<decltype(V)::value, 4, decltype(A)::value, false><<<grid, 256, 0, (hipStream_t)stream>>>(a);
        });
    });
    GNNMP_LAUNCH_CHECK("cg_grad_dst_kernel");
    a.rows = cg_whole_rows(plan_t);      // the same heights: the same geometry and grid
    a.out = job->dfs_j;
    a.dfs_e = nullptr;
    with_vec(vec, [&](auto V) {
        with_cg_act(job->act, [&](auto A) {
            if (has_e)
                cg_grad_src_kernel<decltype(V)::value, 4, decltype(A)::value, true><<<grid, 256, 0, (hipStream_t)stream>>>(a);
            else
                cg_grad_src_kernel<decltype(V)::value, 4, decltype(A)::value, false><<<grid, 256, 0, (hipStream_t)stream>>>(a);
        });
    });
    GNNMP_LAUNCH_CHECK("cg_grad_src_kernel");
    return GNNMP_OK;
}
