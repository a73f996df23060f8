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
// Whole-row walks on the shared pieces and conventions of slotwalk.h (no atomics, every output written once, a hub row by one lane group).
// A kNN graph has no hub destination (every row holds exactly k edges); its SOURCES can be hubs (feature-space kNN has them), so the src
// pass is where the one-lane-group hub row shows.
#include "launch.h"
#include "slotwalk.h"

namespace gnnmp {

struct EdgeConvArgs {
    PlanRows rows;               // forward / dst pass: the plan; src pass: the transposed plan.  Whole rows (plan_rows_whole)
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
    for (uint32_t base = beg; base < end; base += G) {
        const Slots s = load_slots<true, false>(col, nullptr, base, end, lig, G);
        for (int j = 0; j < s.n; j += U) {
            float v[U][VEC];
            int cjs[U];
            bcast_word<U>(s.c, s.n, gbase, j, cjs);
#pragma unroll
            for (int u = 0; u < U; ++u) load_or_zero<VEC>(active, src + (int64_t)cjs[u] * ld, v[u]);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (j + u < s.n) f(v[u]);
            }
        }
    }
}

template <int VEC, int U, int OP, int ACT>
__global__ void __launch_bounds__(256) edge_conv_rows_kernel(const EdgeConvArgs a) {
    RowLane w;
    if (!decode_row_lane<VEC>(a.rows, a.geom, a.C, w)) return;
    const int row = w.row, lig = w.lig, gbase = w.gbase, G = w.G, f0 = w.f0;
    const uint32_t beg = w.beg, end = w.end;
    const bool active = w.active;
    const int64_t ld = 2 * (int64_t)a.C;
    const float *pj = a.p + a.C + f0;      // the x_j share of row 0
    float ai[VEC], acc[VEC];
    {
        float pi[VEC], ps[VEC];
        load_or_zero<VEC>(active, a.p + (int64_t)row * ld + f0, pi);
        load_or_zero<VEC>(active, pj + (int64_t)row * ld, ps);
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
    RowLane w;
    if (!decode_row_lane<VEC>(a.rows, a.geom, a.C, w)) return;
    const int row = w.row, lig = w.lig, gbase = w.gbase, G = w.G, f0 = w.f0;
    const uint32_t beg = w.beg, end = w.end;
    const bool active = w.active;
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
    RowLane w;
    if (!decode_row_lane<VEC>(a.rows, a.geom, a.C, w)) return;
    const int row = w.row, lig = w.lig, gbase = w.gbase, G = w.G, f0 = w.f0;
    const uint32_t beg = w.beg, end = w.end;
    const bool active = w.active;
    const int64_t ld = 2 * (int64_t)a.C;
    float bj[VEC], acc[VEC];
#pragma unroll
    for (int q = 0; q < VEC; ++q) acc[q] = 0.0f;
    load_or_zero<VEC>(NEED_PRE && active, a.p + (int64_t)row * ld + a.C + f0, bj);   // this source's x_j share
    const bool mean = OP == OP_SUM && a.mean;
    for (uint32_t base = beg; base < end; base += G) {
        const Slots s = load_slots<true, false>(a.rows.col, nullptr, base, end, lig, G);      // col: the destination of the edge
        uint32_t cn = 1;
        if (mean && base + lig < end) cn = a.dst_rowptr[s.c + 1] - a.dst_rowptr[s.c];   // >= 1: this edge is in that row
        for (int j = 0; j < s.n; j += U) {
            float pi[NEED_PRE ? U : 1][VEC], ps[NEED_PRE ? U : 1][VEC], yv[OP != OP_SUM ? U : 1][VEC], dv[U][VEC];
            int cjs[U];
            uint32_t cns[U];
            float cnt[U];
            bcast_word<U>(s.c, s.n, gbase, j, cjs);
            if (mean) bcast_word<U>(cn, s.n, gbase, j, cns);
#pragma unroll
            for (int u = 0; u < U; ++u) cnt[u] = mean ? (float)cns[u] : 1.0f;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t ci = cjs[u];
                if (NEED_PRE) {
                    load_or_zero<VEC>(active, a.p + ci * ld + f0, pi[NEED_PRE ? u : 0]);
                    load_or_zero<VEC>(active, a.p + ci * ld + a.C + f0, ps[NEED_PRE ? u : 0]);
                }
                if (OP != OP_SUM) load_or_zero<VEC>(active, a.y + ci * a.C + f0, yv[OP != OP_SUM ? u : 0]);
                load_or_zero<VEC>(active, a.dy + ci * a.C + f0, dv[u]);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (j + u < s.n) {
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
    load_or_zero<VEC>(active, a.out + (int64_t)row * ld + f0, da);   // dA_j, written by the dst pass
#pragma unroll
    for (int q = 0; q < VEC; ++q) acc[q] = acc[q] - da[q];
    if (active) Vec<VEC>::store(a.out + (int64_t)row * ld + a.C + f0, acc);
}

// what both exports check of (plan, C, aggr, act) before any HIP call
static int edge_conv_check(const char *who, const gnnmp_graph_t *plan, const gnnmp_graph_t *plan_t, int64_t C, int aggr, int act) {
    if (C < 1 || C > (1 << 20)) return fail(GNNMP_EINVAL, "%s: bad C %lld", who, (long long)C);
    if (aggr < GNNMP_SUM || aggr > GNNMP_MIN) return fail(GNNMP_EINVAL, "%s: bad aggr %d", who, aggr);
    if (act != GNNMP_ACT_IDENTITY && act != GNNMP_ACT_RELU) return fail(GNNMP_EINVAL, "%s: bad act %d (identity or relu)", who, act);
    return check_edge_plan(who, plan, plan_t, true, nullptr);      // no per-edge array: a plan with self loops of its own is welcome
}

template <class F>
static void with_aggr_act(int aggr, int act, F &&f) {
    const int op = aggr == GNNMP_MAX ? OP_MAX : (aggr == GNNMP_MIN ? OP_MIN : OP_SUM);
    with_op(op, [&](auto O) { with_act<GNNMP_ACT_RELU>(act, [&](auto A) { f(O, A); }); });
}

}  // namespace gnnmp

using namespace gnnmp;

extern "C" int gnnmp_edge_conv_f32(const gnnmp_graph_t *plan, const gnnmp_edge_conv_t *job, int64_t C, gnnmp_stream_t stream) {
    if (!plan) return fail(GNNMP_EINVAL, "edge_conv: null plan");
    if (!job) return fail(GNNMP_EINVAL, "edge_conv: null job");
    if (!job->p) return fail(GNNMP_EINVAL, "edge_conv: null p");
    if (!job->y) return fail(GNNMP_EINVAL, "edge_conv: null y");
    GNNMP_TRY(edge_conv_check("edge_conv", plan, nullptr, C, job->aggr, job->act));
    if (plan->n_dst == 0) return GNNMP_OK;
    EdgeConvArgs a = {};
    a.rows = plan_rows_whole(plan);
    a.p = job->p;
    a.out = job->y;
    a.C = (int)C;
    a.mean = job->aggr == GNNMP_MEAN;
    dim3 grid;
    const int vec = row_walk_geom("edge_conv", a.rows, C, 0, {job->p, job->y}, a.geom, grid);
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
    GNNMP_TRY(edge_conv_check("edge_conv_grad", plan, plan_t, C, job->aggr, job->act));
    if (plan->n_dst == 0) return GNNMP_OK;
    EdgeConvArgs a = {};
    a.rows = plan_rows_whole(plan);
    a.p = job->p;
    a.y = job->y;
    a.dy = job->dy;
    a.out = job->dp;
    a.dst_rowptr = plan->rowptr;
    a.C = (int)C;
    a.mean = job->aggr == GNNMP_MEAN;
    dim3 grid;
    const int vec = row_walk_geom("edge_conv_grad", a.rows, C, 0, {job->p, job->y, job->dy, job->dp}, a.geom, grid);
    if (vec < 0) return vec;
    auto launch = [&](bool src) {      // the dst pass over a.rows = the plan, then the src pass over the transposed plan
        with_vec(vec, [&](auto V) {
            with_aggr_act(job->aggr, job->act, [&](auto O, auto A) {
                constexpr int VEC = decltype(V)::value, OP = decltype(O)::value, ACT = decltype(A)::value;
                if (src)
                    edge_conv_grad_src_kernel<VEC, 4, OP, ACT><<<grid, 256, 0, (hipStream_t)stream>>>(a);
                else
                    edge_conv_grad_dst_kernel<VEC, 8, OP, ACT><<<grid, 256, 0, (hipStream_t)stream>>>(a);
            });
        });
    };
    launch(false);
    GNNMP_LAUNCH_CHECK("edge_conv_grad_dst_kernel");
    a.rows = plan_rows_whole(plan_t);      // the same heights: the same geometry and grid
    launch(true);
    GNNMP_LAUNCH_CHECK("edge_conv_grad_src_kernel");
    return GNNMP_OK;
}
