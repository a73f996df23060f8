// edge_conv.hip — EdgeConv with a one-layer nn, forward and pullback, as passes of a row kernel over gathered rows of a NODE-level matrix.
// edge_conv (GNNlib/src/layers/conv.jl:237-246) is propagate(edge_conv_message, g, aggr) with the message nn(vcat(xi, xj .- xi)).  For
// nn = Dense(2D => C, σ), W = [W1 | W2], the contraction leaves the edges:
//     nn(vcat(xi, xj - xi)) = σ(W1 xi + b - W2 xi + W2 xj)
// so ONE dense call on N rows gives P = x [W1; W2]ᵀ + [b; 0], [N][2C] planar (columns [0, C): the x_i share with the bias, columns
// [C, 2C): the x_j share — the per-edge gather fetches only the second half of a row), and what is left per edge is two additions and σ:
//     a_i[c]   = P[i][c] - P[i][C + c]        once per destination row, kept in registers
//     pre_e[c] = a_i[c] + P[j][C + c]
//     m_e[c]   = σ(pre_e[c])                  σ: identity | relu
//     y_i[c]   = aggr_e m_e[c]                + | mean | max | min, folded in ORIGINAL edge order from the operator's identity
// Nothing of E rows is ever written, forward or backward.  Three kernels on the conventions of rowwalk.h:
//   edge_conv_rows_kernel       a lane group (16 bytes a lane) owns destination i, walks its row of the plan with U gathered rows of P in
//                               flight (column indices one per lane, shuffled), writes y[i] once
//   edge_conv_grad_dst_kernel   the same walk: dP[i][0..C) = dA_i = Σ_{e into i} g_e
//   edge_conv_grad_src_kernel   walks the TRANSPOSED plan (row j: the edges that leave j, in edge order), gathers per edge what it needs
//                               of the destination i (P[i], y[i], Δ[i], count_i): dB_j = Σ_{e out of j} g_e, and writes
//                               dP[j][C..2C) = dB_j - dP[j][0..C) — it runs after the dst pass on the same stream
// with  r_e = Δ_i (+) | Δ_i / count_i (mean) | (m_e == y_i ? Δ_i : 0) (max / min: EVERY maximiser receives Δ, as maxmin_grad.h),
//       g_e = r_e (identity) | (pre_e > 0 ? r_e : 0) (relu: 0 at 0, as gnnmp_act_grad_f32).
// pre_e and m_e are RECOMPUTED in both gradient passes with exactly the two operations above: the tie test is an equality on floats, a
// differently associated recomputation would be a wrong gradient.  What a pass does not need it does not load (+ / mean with σ =
// identity: g_e = r_e, no row of P is gathered).
//
// No atomics, no plan-owned scratch, every output element written exactly once (rows without in-edges and rows without out-edges
// included).  All three kernels walk every ordinary row WHOLE, in edge order, whatever its length: their PlanRows carries n_chunks = 0
// and decode_vrow is told not to skip long rows (VROW_WHOLE) — as hetero_rows_kernel / hetero_grad_rows_kernel do.  Every row therefore
// has the bits of the sequential fold; the price is that A HUB ROW IS WALKED BY ONE LANE GROUP: correct, slow.  A kNN graph has no hub
// destination (every row holds exactly k edges); its SOURCES can be hubs (feature-space kNN has them), so the src pass is where that
// shows.  Chunked hub rows are a later change.
#include "rowwalk.h"

namespace gnnmp {

struct EdgeConvArgs {
    PlanRows rows;               // forward / dst pass: the plan; src pass: the transposed plan.  n_chunks = 0 (rows are walked whole)
    RowGeom geom;
    const float *p;              // [n][2C]
    const float *y;              // [n][C] the forward output (gradient passes, max / min)
    const float *dy;             // [n][C]
    float *out;                  // forward: y [n][C]; gradient passes: dp [n][2C]
    const uint32_t *dst_rowptr;  // src pass, mean: the FORWARD plan's rowptr — count_i of a gathered destination
    int C;
    int mean;                    // OP_SUM instances: divide by the row's edge count
};

template <int ACT>
__device__ __forceinline__ float edge_conv_act(float pre) {
    return ACT == GNNMP_ACT_RELU ? (pre < 0.0f ? 0.0f : pre) : pre;
}
// g_e from the recomputed pre_e, the destination's y and Δ (r_sum: Δ_i, or Δ_i / count_i for mean)
template <int OP, int ACT>
__device__ __forceinline__ float edge_conv_g(float pre, float yv, float dv, float r_sum) {
    const float r = OP == OP_SUM ? r_sum : (edge_conv_act<ACT>(pre) == yv ? dv : 0.0f);
    return ACT == GNNMP_ACT_RELU ? (pre > 0.0f ? r : 0.0f) : r;
}

// Slots [beg, end) of one row, in order: U gathered rows src[col_p * ld ...] (src already points at the lane's features) in flight per
// lane group, column indices one per lane and shuffled, f(v) once per slot.  All lanes of the group call this together.
template <int VEC, int U, class F>
__device__ __forceinline__ void edge_conv_walk(const int32_t *col, const float *src, int64_t ld, uint32_t beg, uint32_t end, int lig, int gbase,
                                               int G, bool active, F &&f) {
    for (uint32_t base = beg; base < end; base += G) {   // slots are unsigned 32-bit (rowwalk.h)
        const uint32_t p = base + lig;
        const int c = p < end ? col[p] : 0;
        const int n = (int)min((uint32_t)G, end - base);
        for (int j = 0; j < n; j += U) {
            float v[U][VEC];
            int cjs[U];
#pragma unroll
            for (int u = 0; u < U; ++u) cjs[u] = __shfl(c, gbase + min(j + u, n - 1), 64);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (active) {   // clamped, unconditional within the lane's activity (maxmin_grad.h)
                    Vec<VEC>::load(src + (int64_t)cjs[u] * ld, v[u]);
                } else {
#pragma unroll
                    for (int q = 0; q < VEC; ++q) v[u][q] = 0.0f;
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (j + u < n) f(v[u]);
            }
        }
    }
}

template <int VEC, int U, int OP, int ACT>
__global__ void __launch_bounds__(256) edge_conv_rows_kernel(const EdgeConvArgs a) {
    VRow vr;
    if (!decode_vrow<VROW_WHOLE>(a.rows, a.geom, blockIdx.x, vr)) return;
    const int row = vr.row, lig = vr.lig, gbase = vr.gbase, G = vr.G;
    const uint32_t beg = vr.beg, end = vr.end;
    const int f0 = ((int)blockIdx.y * G + lig) * VEC;
    const bool active = f0 < a.C;
    const int64_t ld = 2 * (int64_t)a.C;
    const float *pj = a.p + a.C + f0;      // the x_j share of row 0
    float ai[VEC], acc[VEC];
    {
        float pi[VEC], ps[VEC];
#pragma unroll
        for (int q = 0; q < VEC; ++q) pi[q] = ps[q] = 0.0f;
        if (active) {
            Vec<VEC>::load(a.p + (int64_t)row * ld + f0, pi);
            Vec<VEC>::load(pj + (int64_t)row * ld, ps);
        }
#pragma unroll
        for (int q = 0; q < VEC; ++q) {
            ai[q] = pi[q] - ps[q];
            acc[q] = op_identity<OP>();
        }
    }
    edge_conv_walk<VEC, U>(a.rows.col, pj, ld, beg, end, lig, gbase, G, active, [&](const float v[VEC]) {
#pragma unroll
        for (int q = 0; q < VEC; ++q) acc[q] = op_apply<OP>(acc[q], edge_conv_act<ACT>(ai[q] + v[q]));
    });
    if (OP == OP_SUM && a.mean) {   // NNlib scatter(mean): 0 .+ safe_div.(sum, count), as finalize_row (csr_reduce.h)
        const uint32_t len = end - beg;
        const float cnt = (float)len;
#pragma unroll
        for (int q = 0; q < VEC; ++q) acc[q] = 0.0f + (len == 0 ? acc[q] : acc[q] / cnt);
    }
    if (active) Vec<VEC>::store(a.out + (int64_t)row * a.C + f0, acc);
}

template <int VEC, int U, int OP, int ACT>
__global__ void __launch_bounds__(256) edge_conv_grad_dst_kernel(const EdgeConvArgs a) {
    constexpr bool NEED_PRE = ACT == GNNMP_ACT_RELU || OP != OP_SUM;
    VRow vr;
    if (!decode_vrow<VROW_WHOLE>(a.rows, a.geom, blockIdx.x, vr)) return;
    const int row = vr.row, lig = vr.lig, gbase = vr.gbase, G = vr.G;
    const uint32_t beg = vr.beg, end = vr.end;
    const int f0 = ((int)blockIdx.y * G + lig) * VEC;
    const bool active = f0 < a.C;
    const int64_t ld = 2 * (int64_t)a.C;
    const float *pj = a.p + a.C + f0;
    float ai[VEC], yv[VEC], dv[VEC], rs[VEC], acc[VEC];
    {
        float pi[VEC], ps[VEC];
#pragma unroll
        for (int q = 0; q < VEC; ++q) pi[q] = ps[q] = yv[q] = dv[q] = 0.0f;
        if (active) {
            if (NEED_PRE) {
                Vec<VEC>::load(a.p + (int64_t)row * ld + f0, pi);
                Vec<VEC>::load(pj + (int64_t)row * ld, ps);
            }
            if (OP != OP_SUM) Vec<VEC>::load(a.y + (int64_t)row * a.C + f0, yv);
            Vec<VEC>::load(a.dy + (int64_t)row * a.C + f0, dv);
        }
        const float cnt = (float)max(end - beg, 1u);
#pragma unroll
        for (int q = 0; q < VEC; ++q) {
            ai[q] = pi[q] - ps[q];
            rs[q] = (OP == OP_SUM && a.mean) ? dv[q] / cnt : dv[q];   // mean: divided once per row
            acc[q] = 0.0f;
        }
    }
    if (!NEED_PRE) {   // g_e = r_e for every edge: the row's sum of equal terms, added one by one as the sequential fold does
        for (uint32_t e = beg; e < end; ++e) {
#pragma unroll
            for (int q = 0; q < VEC; ++q) acc[q] = acc[q] + rs[q];
        }
    } else {
        edge_conv_walk<VEC, U>(a.rows.col, pj, ld, beg, end, lig, gbase, G, active, [&](const float v[VEC]) {
#pragma unroll
            for (int q = 0; q < VEC; ++q) acc[q] = acc[q] + edge_conv_g<OP, ACT>(ai[q] + v[q], yv[q], dv[q], rs[q]);
        });
    }
    if (active) Vec<VEC>::store(a.out + (int64_t)row * ld + f0, acc);
}

template <int VEC, int U, int OP, int ACT>
__global__ void __launch_bounds__(256) edge_conv_grad_src_kernel(const EdgeConvArgs a) {
    constexpr bool NEED_PRE = ACT == GNNMP_ACT_RELU || OP != OP_SUM;
    VRow vr;
    if (!decode_vrow<VROW_WHOLE>(a.rows, a.geom, blockIdx.x, vr)) return;
    const int row = vr.row, lig = vr.lig, gbase = vr.gbase, G = vr.G;
    const uint32_t beg = vr.beg, end = vr.end;
    const int f0 = ((int)blockIdx.y * G + lig) * VEC;
    const bool active = f0 < a.C;
    const int64_t ld = 2 * (int64_t)a.C;
    float bj[VEC], acc[VEC];
#pragma unroll
    for (int q = 0; q < VEC; ++q) bj[q] = acc[q] = 0.0f;
    if (NEED_PRE && active) Vec<VEC>::load(a.p + (int64_t)row * ld + a.C + f0, bj);   // this source's x_j share
    const bool mean = OP == OP_SUM && a.mean;
    for (uint32_t base = beg; base < end; base += G) {
        const uint32_t p = base + lig;
        int c = 0;
        uint32_t cn = 1;
        if (p < end) {
            c = a.rows.col[p];                                  // the destination of the edge
            if (mean) cn = a.dst_rowptr[c + 1] - a.dst_rowptr[c];   // >= 1: this edge is in that row
        }
        const int n = (int)min((uint32_t)G, end - base);
        for (int j = 0; j < n; j += U) {
            float pi[NEED_PRE ? U : 1][VEC], ps[NEED_PRE ? U : 1][VEC], yv[OP != OP_SUM ? U : 1][VEC], dv[U][VEC];
            int cjs[U];
            float cnt[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int jj = min(j + u, n - 1);
                cjs[u] = __shfl(c, gbase + jj, 64);
                cnt[u] = mean ? (float)(uint32_t)__shfl((int)cn, gbase + jj, 64) : 1.0f;
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t ci = cjs[u];
                if (active) {
                    if (NEED_PRE) {
                        Vec<VEC>::load(a.p + ci * ld + f0, pi[NEED_PRE ? u : 0]);
                        Vec<VEC>::load(a.p + ci * ld + a.C + f0, ps[NEED_PRE ? u : 0]);
                    }
                    if (OP != OP_SUM) Vec<VEC>::load(a.y + ci * a.C + f0, yv[OP != OP_SUM ? u : 0]);
                    Vec<VEC>::load(a.dy + ci * a.C + f0, dv[u]);
                } else {
#pragma unroll
                    for (int q = 0; q < VEC; ++q) {
                        if (NEED_PRE) pi[NEED_PRE ? u : 0][q] = ps[NEED_PRE ? u : 0][q] = 0.0f;
                        if (OP != OP_SUM) yv[OP != OP_SUM ? u : 0][q] = 0.0f;
                        dv[u][q] = 0.0f;
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (j + u < n) {
#pragma unroll
                    for (int q = 0; q < VEC; ++q) {
                        const float d = dv[u][q];
                        const float rs = mean ? d / cnt[u] : d;
                        float pre = 0.0f, yy = 0.0f;
                        if (NEED_PRE) pre = (pi[NEED_PRE ? u : 0][q] - ps[NEED_PRE ? u : 0][q]) + bj[q];   // a_i, then pre_e
                        if (OP != OP_SUM) yy = yv[OP != OP_SUM ? u : 0][q];
                        acc[q] = acc[q] + edge_conv_g<OP, ACT>(pre, yy, d, rs);
                    }
                }
            }
        }
    }
    float da[VEC];
#pragma unroll
    for (int q = 0; q < VEC; ++q) da[q] = 0.0f;
    if (active) Vec<VEC>::load(a.out + (int64_t)row * ld + f0, da);   // dA_j, written by the dst pass
#pragma unroll
    for (int q = 0; q < VEC; ++q) acc[q] = acc[q] - da[q];
    if (active) Vec<VEC>::store(a.out + (int64_t)row * ld + a.C + f0, acc);
}

// what both exports check of (plan, C, aggr, act) before any HIP call
static int edge_conv_check(const char *who, const gnnmp_graph_t *plan, int64_t C, int aggr, int act) {
    if (C < 1 || C > (1 << 20)) return fail(GNNMP_EINVAL, "%s: bad C %lld", who, (long long)C);
    if (aggr < GNNMP_SUM || aggr > GNNMP_MIN) return fail(GNNMP_EINVAL, "%s: bad aggr %d", who, aggr);
    if (act != GNNMP_ACT_IDENTITY && act != GNNMP_ACT_RELU) return fail(GNNMP_EINVAL, "%s: bad act %d (identity or relu)", who, act);
    if (plan->n_src != plan->n_dst)
        return fail(GNNMP_EINVAL, "%s: the plan is not square (%lld sources, %lld destinations)", who, (long long)plan->n_src, (long long)plan->n_dst);
    return GNNMP_OK;
}

// the vector width every array of a call admits, and the row walk's geometry for it
static int edge_conv_geom(const char *who, EdgeConvArgs &a, uintptr_t align, dim3 &grid) {
    const int vec = pick_vec(a.C, reinterpret_cast<const void *>(align), nullptr);
    a.geom = RowGeom{pick_log2g((a.C + vec - 1) / vec), 4, 0, 0};
    if (row_blocks(a.rows, a.geom) >= INT32_MAX) return fail(GNNMP_EUNSUPPORTED, "%s: too many row blocks", who);
    grid = row_grid(a.rows, a.geom, feature_tiles(a.C, vec, a.geom.log2g));
    return vec;
}

static PlanRows whole_rows(const gnnmp_graph_t *plan) {
    PlanRows r = plan_rows(plan);
    r.n_chunks = 0;     // no chunk virtual rows: VROW_WHOLE walks the long rows themselves
    r.n_long = 0;
    return r;
}

template <class F>
static void with_aggr_act(int aggr, int act, F &&f) {
    const int op = aggr == GNNMP_MAX ? OP_MAX : (aggr == GNNMP_MIN ? OP_MIN : OP_SUM);
    with_op(op, [&](auto O) {
        if (act == GNNMP_ACT_RELU)
            f(O, int_c<GNNMP_ACT_RELU>{});
        else
            f(O, int_c<GNNMP_ACT_IDENTITY>{});
    });
}

}  // namespace gnnmp

using namespace gnnmp;

extern "C" int gnnmp_edge_conv_f32(const gnnmp_graph_t *plan, const gnnmp_edge_conv_t *job, int64_t C, gnnmp_stream_t stream) {
    if (!plan) return fail(GNNMP_EINVAL, "edge_conv: null plan");
    if (!job) return fail(GNNMP_EINVAL, "edge_conv: null job");
    if (!job->p) return fail(GNNMP_EINVAL, "edge_conv: null p");
    if (!job->y) return fail(GNNMP_EINVAL, "edge_conv: null y");
    GNNMP_TRY(edge_conv_check("edge_conv", plan, C, job->aggr, job->act));
    if (plan->n_dst == 0) return GNNMP_OK;
    EdgeConvArgs a = {};
    a.rows = whole_rows(plan);
    a.p = job->p;
    a.out = job->y;
    a.C = (int)C;
    a.mean = job->aggr == GNNMP_MEAN;
    // 16 / 8-byte lanes need C % 4 / C % 2 == 0 and every pointer aligned alike — p + C, column C inside a row, included
    dim3 grid;
    const int vec = edge_conv_geom("edge_conv", a, reinterpret_cast<uintptr_t>(job->p) | reinterpret_cast<uintptr_t>(job->p + C) |
                                                       reinterpret_cast<uintptr_t>(job->y), grid);
    if (vec < 0) return vec;
    with_vec(vec, [&](auto V) {
        with_aggr_act(job->aggr, job->act, [&](auto O, auto A) {
            edge_conv_rows_kernel<decltype(V)::value, 8, decltype(O)::value, decltype(A)::value><<<grid, 256, 0, (hipStream_t)stream>>>(a);
        });
    });
    GNNMP_LAUNCH_CHECK("edge_conv_rows_kernel");
    return GNNMP_OK;
}

extern "C" int gnnmp_edge_conv_grad_f32(const gnnmp_graph_t *plan, const gnnmp_graph_t *plan_t, const gnnmp_edge_conv_grad_t *job, int64_t C,
                                        gnnmp_stream_t stream) {
    if (!plan) return fail(GNNMP_EINVAL, "edge_conv_grad: null plan");
    if (!plan_t) return fail(GNNMP_EINVAL, "edge_conv_grad: null plan_t");
    if (!job) return fail(GNNMP_EINVAL, "edge_conv_grad: null job");
    if (!job->p) return fail(GNNMP_EINVAL, "edge_conv_grad: null p");
    if (!job->y) return fail(GNNMP_EINVAL, "edge_conv_grad: null y");
    if (!job->dy) return fail(GNNMP_EINVAL, "edge_conv_grad: null dy");
    if (!job->dp) return fail(GNNMP_EINVAL, "edge_conv_grad: null dp");
    GNNMP_TRY(edge_conv_check("edge_conv_grad", plan, C, job->aggr, job->act));
    if (plan_t->n_dst != plan->n_dst || plan_t->n_src != plan->n_src)
        return fail(GNNMP_EINVAL, "edge_conv_grad: the transposed plan has %lld rows, the plan %lld", (long long)plan_t->n_dst, (long long)plan->n_dst);
    if (plan_t->n_edges != plan->n_edges || plan_t->n_total != plan->n_total)
        return fail(GNNMP_EINVAL, "edge_conv_grad: the transposed plan has %lld edges, the plan %lld", (long long)plan_t->n_total, (long long)plan->n_total);
    if (plan->n_dst == 0) return GNNMP_OK;
    EdgeConvArgs a = {};
    a.rows = whole_rows(plan);
    a.p = job->p;
    a.y = job->y;
    a.dy = job->dy;
    a.out = job->dp;
    a.dst_rowptr = plan->rowptr;
    a.C = (int)C;
    a.mean = job->aggr == GNNMP_MEAN;
    dim3 grid;
    const int vec = edge_conv_geom("edge_conv_grad", a, reinterpret_cast<uintptr_t>(job->p) | reinterpret_cast<uintptr_t>(job->p + C) |
                                                            reinterpret_cast<uintptr_t>(job->y) | reinterpret_cast<uintptr_t>(job->dy) |
                                                            reinterpret_cast<uintptr_t>(job->dp) | reinterpret_cast<uintptr_t>(job->dp + C), grid);
    if (vec < 0) return vec;
    with_vec(vec, [&](auto V) {
        with_aggr_act(job->aggr, job->act, [&](auto O, auto A) {
            edge_conv_grad_dst_kernel<decltype(V)::value, 8, decltype(O)::value, decltype(A)::value><<<grid, 256, 0, (hipStream_t)stream>>>(a);
        });
    });
    GNNMP_LAUNCH_CHECK("edge_conv_grad_dst_kernel");
    a.rows = whole_rows(plan_t);      // the same heights: the same geometry and grid
    with_vec(vec, [&](auto V) {
        with_aggr_act(job->aggr, job->act, [&](auto O, auto A) {
            edge_conv_grad_src_kernel<decltype(V)::value, 4, decltype(O)::value, decltype(A)::value><<<grid, 256, 0, (hipStream_t)stream>>>(a);
        });
    });
    GNNMP_LAUNCH_CHECK("edge_conv_grad_src_kernel");
    return GNNMP_OK;
}
