// megnet.hip — the E-row steps of MEGNetConv's training path (megnet_conv, GNNlib/src/layers/conv.jl:356-368) that no other export gives,
// as row kernels: the per-edge hidden layer act(P_i + Q_j + F_k) with its pullback to the destination, the source and the edge at once,
// and the pullback of aggregate_neighbors (msgpass.jl:145-149) for all four folds.  Edge k: j -> i (include/gnnmp.h states the arithmetic).
//   megnet_edge_kernel       a lane group owns destination i, keeps P_i in registers, walks its row of the plan: gathers Q[col] and
//                            F[eid], z0_k = (P_i + Q_j) + F_k, a0_k = act(z0_k) by bias_act_apply — the device function of
//                            gnnmp_bias_act_f32 — stored at row eid (the original edge position; every edge lies in exactly one row, so
//                            every element of a0 / z0 is written exactly once)
//   megnet_edge_grad_kernel  dz0_k = da0_k ⊙ act'(z_k) by act_dz — the device function of gnnmp_act_grad_z_f32.  Over the plan: dz0 at
//                            row eid when wanted, dP_i = Σ_{k into i} dz0_k; the same kernel over the TRANSPOSED plan recomputes dz0_k
//                            from da0[eid], z[eid] and gives dQ_j = Σ_{k out of j} dz0_k.  It reads eid only, never col.
//   aggregate_grad_kernel    dy_i (and, for max / min, y_i) in registers; per slot the term dy_i | dy_i / deg_i | (m_k == y_i ? dy_i : 0),
//                            dm[eid] = (acc[eid] +) term
// Whole-row walks on the shared pieces and conventions of slotwalk.h (no atomics, every output written once, a hub row by one lane group).
//
// Registers: U = 4 slots in flight; per slot the edge kernel gathers two vectors, the pullback two, the aggregate pullback two — at most
// 32 VGPRs of loads with 16-byte lanes.  The compiler's resource report (LABNOTES.md) shows no scratch for any instance.
#include "csr_reduce.h"
#include "launch.h"

namespace gnnmp {

struct MegnetEdgeArgs {
    PlanRows rows;               // the plan, whole rows (plan_rows_whole)
    RowGeom geom;
    const float *P, *Q;          // [n][hid]
    const float *F;              // [n_edges][hid], read by the HAS_F instances only
    float *a0;                   // [n_edges][hid]
    float *z0;                   // [n_edges][hid] or null
    int hid;
};

template <int VEC, int U, int ACT, bool HAS_F>
__global__ void __launch_bounds__(256) megnet_edge_kernel(const MegnetEdgeArgs a) {
    RowLane w;
    if (!decode_row_lane<VEC>(a.rows, a.geom, a.hid, w)) return;
    const int f0 = w.f0;
    const bool active = w.active;
    const int64_t ld = a.hid;
    float pi[VEC];
    load_or_zero<VEC>(active, a.P + (int64_t)w.row * ld + f0, pi);
    const bool store_z = a.z0 != nullptr;
    for (uint32_t base = w.beg; base < w.end; base += w.G) {
        const Slots s = load_slots<true, true>(a.rows.col, a.rows.eid, base, w.end, w.lig, w.G);
        for (int j = 0; j < s.n; j += U) {
            float qj[U][VEC], fe[HAS_F ? U : 1][VEC];
            int cjs[U];
            uint32_t ejs[U];
            bcast_slots<U, true, true>(s, w.gbase, j, cjs, ejs);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                load_or_zero<VEC>(active, a.Q + (int64_t)cjs[u] * ld + f0, qj[u]);
                if (HAS_F) load_or_zero<VEC>(active, a.F + (int64_t)ejs[u] * ld + f0, fe[HAS_F ? u : 0]);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (j + u < s.n && active) {
                    float z[VEC], y[VEC];
#pragma unroll
                    for (int q = 0; q < VEC; ++q) {
                        z[q] = pi[q] + qj[u][q];
                        if (HAS_F) z[q] = z[q] + fe[HAS_F ? u : 0][q];
                        y[q] = bias_act_apply(z[q], ACT);
                    }
                    if (store_z) Vec<VEC>::store(a.z0 + (int64_t)ejs[u] * ld + f0, z);
                    Vec<VEC>::store(a.a0 + (int64_t)ejs[u] * ld + f0, y);
                }
            }
        }
    }
}

struct MegnetGradArgs {
    PlanRows rows;               // pass 1: the plan; pass 2: the transposed plan.  Whole rows
    RowGeom geom;
    const float *da0;            // [n_edges][hid]
    const float *z;              // [n_edges][hid]; not read by the IDENTITY instances
    float *dz0;                  // pass 1: [n_edges][hid] or null; pass 2: null
    float *out;                  // pass 1: dP [n][hid] or null; pass 2: dQ [n][hid]
    int hid;
};

template <int VEC, int U, int ACT>
__global__ void __launch_bounds__(256) megnet_edge_grad_kernel(const MegnetGradArgs a) {
    RowLane w;
    if (!decode_row_lane<VEC>(a.rows, a.geom, a.hid, w)) return;
    const int f0 = w.f0;
    const bool active = w.active;
    const int64_t ld = a.hid;
    constexpr bool HAS_Z = ACT != GNNMP_ACT_IDENTITY;
    float acc[VEC];
#pragma unroll
    for (int q = 0; q < VEC; ++q) acc[q] = 0.0f;
    const bool store_e = a.dz0 != nullptr;
    for (uint32_t base = w.beg; base < w.end; base += w.G) {
        const Slots s = load_slots<false, true>(a.rows.col, a.rows.eid, base, w.end, w.lig, w.G);
        for (int j = 0; j < s.n; j += U) {
            float da[U][VEC], zv[HAS_Z ? U : 1][VEC];
            uint32_t ejs[U];
            bcast_word<U>(s.ev, s.n, w.gbase, j, ejs);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (active) {      // one branch round both loads: load_or_zero per load costs <4, 4, SOFTPLUS | SWISH> a wave (LABNOTES.md)
                    Vec<VEC>::load(a.da0 + (int64_t)ejs[u] * ld + f0, da[u]);
                    if (HAS_Z) Vec<VEC>::load(a.z + (int64_t)ejs[u] * ld + f0, zv[HAS_Z ? u : 0]);
                } else {
#pragma unroll
                    for (int q = 0; q < VEC; ++q) {
                        da[u][q] = 0.0f;
                        if (HAS_Z) zv[HAS_Z ? u : 0][q] = 0.0f;
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (j + u < s.n) {
                    float d[VEC];
#pragma unroll
                    for (int q = 0; q < VEC; ++q) {
                        d[q] = act_dz<ACT>(da[u][q], HAS_Z ? zv[HAS_Z ? u : 0][q] : 0.0f);
                        acc[q] = acc[q] + d[q];
                    }
                    if (store_e && active) Vec<VEC>::store(a.dz0 + (int64_t)ejs[u] * ld + f0, d);
                }
            }
        }
    }
    if (a.out != nullptr && active) Vec<VEC>::store(a.out + (int64_t)w.row * ld + f0, acc);
}

struct AggrGradArgs {
    PlanRows rows;               // the plan, whole rows
    RowGeom geom;
    const float *dy;             // [n_dst][D]
    const float *m, *y;          // [n_edges][D], [n_dst][D]: read by the SEL (max / min) instances only
    const float *acc;            // [n_edges][D], read by the HAS_ACC instances only
    float *dm;                   // [n_edges][D]
    int D, mean;
};

template <int VEC, int U, bool SEL, bool HAS_ACC>
__global__ void __launch_bounds__(256) aggregate_grad_kernel(const AggrGradArgs a) {
    RowLane w;
    if (!decode_row_lane<VEC>(a.rows, a.geom, a.D, w)) return;
    const int f0 = w.f0;
    const bool active = w.active;
    const int64_t ld = a.D;
    float dv[VEC], yv[VEC];
#pragma unroll
    for (int q = 0; q < VEC; ++q) dv[q] = yv[q] = 0.0f;
    if (active && w.end > w.beg) {
        Vec<VEC>::load(a.dy + (int64_t)w.row * ld + f0, dv);
        if (SEL) Vec<VEC>::load(a.y + (int64_t)w.row * ld + f0, yv);
        if (a.mean) {            // divided once per row
            const float fdeg = (float)(w.end - w.beg);
#pragma unroll
            for (int q = 0; q < VEC; ++q) dv[q] = dv[q] / fdeg;
        }
    }
    for (uint32_t base = w.beg; base < w.end; base += w.G) {
        const Slots s = load_slots<false, true>(a.rows.col, a.rows.eid, base, w.end, w.lig, w.G);
        for (int j = 0; j < s.n; j += U) {
            float mv[SEL ? U : 1][VEC], av[HAS_ACC ? U : 1][VEC];
            uint32_t ejs[U];
            bcast_word<U>(s.ev, s.n, w.gbase, j, ejs);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (SEL) load_or_zero<VEC>(active, a.m + (int64_t)ejs[u] * ld + f0, mv[SEL ? u : 0]);
                if (HAS_ACC) load_or_zero<VEC>(active, a.acc + (int64_t)ejs[u] * ld + f0, av[HAS_ACC ? u : 0]);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (j + u < s.n && active) {
                    float o[VEC];
#pragma unroll
                    for (int q = 0; q < VEC; ++q) {
                        float term = dv[q];
                        if (SEL) term = mv[SEL ? u : 0][q] == yv[q] ? dv[q] : 0.0f;      // every tying copy gets the whole Δ
                        o[q] = HAS_ACC ? av[HAS_ACC ? u : 0][q] + term : term;
                    }
                    Vec<VEC>::store(a.dm + (int64_t)ejs[u] * ld + f0, o);
                }
            }
        }
    }
}

}  // namespace gnnmp

using namespace gnnmp;

extern "C" int gnnmp_megnet_edge_f32(const gnnmp_graph_t *plan, const gnnmp_megnet_edge_t *job, int64_t hid, gnnmp_stream_t stream) {
    if (!plan) return fail(GNNMP_EINVAL, "megnet_edge: null plan");
    if (!job) return fail(GNNMP_EINVAL, "megnet_edge: null job");
    if (!job->P) return fail(GNNMP_EINVAL, "megnet_edge: null P");
    if (!job->Q) return fail(GNNMP_EINVAL, "megnet_edge: null Q");
    if (!job->a0 && plan->n_total > 0) return fail(GNNMP_EINVAL, "megnet_edge: null a0");      // no edge: no row of a0 is written
    if (hid < 1 || hid > (1 << 19)) return fail(GNNMP_EINVAL, "megnet_edge: bad hid %lld", (long long)hid);
    if (job->act < GNNMP_ACT_IDENTITY || job->act > GNNMP_ACT_SWISH) return fail(GNNMP_EINVAL, "megnet_edge: bad act %d", job->act);
    GNNMP_TRY(check_edge_plan("megnet_edge", plan, nullptr, true, "the E-row arrays have no row for them"));
    if (plan->n_dst == 0 || plan->n_total == 0) return GNNMP_OK;
    MegnetEdgeArgs a = {};
    a.rows = plan_rows_whole(plan);
    a.P = job->P;
    a.Q = job->Q;
    a.F = job->F;
    a.a0 = job->a0;
    a.z0 = job->z0;
    a.hid = (int)hid;
    dim3 grid;
    const int vec = row_walk_geom("megnet_edge", a.rows, hid, 0, {job->P, job->Q, job->F, job->a0, job->z0}, a.geom, grid);
    if (vec < 0) return vec;
    const bool has_f = job->F != nullptr;
    with_vec(vec, [&](auto V) {
        with_act<GNNMP_ACT_SWISH>(job->act, [&](auto A) {
            if (has_f)
                megnet_edge_kernel<decltype(V)::value, 4, decltype(A)::value, true><<<grid, 256, 0, (hipStream_t)stream>>>(a);
            else
                megnet_edge_kernel<decltype(V)::value, 4, decltype(A)::value, false><<<grid, 256, 0, (hipStream_t)stream>>>(a);
        });
    });
    GNNMP_LAUNCH_CHECK("megnet_edge_kernel");
    return GNNMP_OK;
}

extern "C" int gnnmp_megnet_edge_grad_f32(const gnnmp_graph_t *plan, const gnnmp_graph_t *plan_t, const gnnmp_megnet_edge_grad_t *job,
                                          int64_t hid, gnnmp_stream_t stream) {
    if (!plan) return fail(GNNMP_EINVAL, "megnet_edge_grad: null plan");
    if (!job) return fail(GNNMP_EINVAL, "megnet_edge_grad: null job");
    if (!job->dz0 && !job->dP && !job->dQ) return fail(GNNMP_EINVAL, "megnet_edge_grad: dz0, dP and dQ are all null");
    if ((job->dP != nullptr) != (job->dQ != nullptr)) return fail(GNNMP_EINVAL, "megnet_edge_grad: dP and dQ come together");
    if (job->dQ && !plan_t) return fail(GNNMP_EINVAL, "megnet_edge_grad: null plan_t");
    if (hid < 1 || hid > (1 << 19)) return fail(GNNMP_EINVAL, "megnet_edge_grad: bad hid %lld", (long long)hid);
    if (job->act < GNNMP_ACT_IDENTITY || job->act > GNNMP_ACT_SWISH) return fail(GNNMP_EINVAL, "megnet_edge_grad: bad act %d", job->act);
    if (plan->n_total > 0) {      // no edge: no row of an E-row array is touched
        if (!job->da0) return fail(GNNMP_EINVAL, "megnet_edge_grad: null da0");
        if (job->act != GNNMP_ACT_IDENTITY && !job->z) return fail(GNNMP_EINVAL, "megnet_edge_grad: null z");
    }
    GNNMP_TRY(check_edge_plan("megnet_edge_grad", plan, job->dQ ? plan_t : nullptr, true, "the E-row arrays have no row for them"));
    if (plan->n_dst == 0) return GNNMP_OK;
    if (plan->n_total == 0 && !job->dP) return GNNMP_OK;
    MegnetGradArgs a = {};
    a.rows = plan_rows_whole(plan);
    a.da0 = job->da0;
    a.z = job->act != GNNMP_ACT_IDENTITY ? job->z : nullptr;
    a.dz0 = plan->n_total > 0 ? job->dz0 : nullptr;
    a.out = job->dP;
    a.hid = (int)hid;
    dim3 grid;
    const int vec = row_walk_geom("megnet_edge_grad", a.rows, hid, 0, {a.da0, a.z, job->dz0, job->dP, job->dQ}, a.geom, grid);
    if (vec < 0) return vec;
    auto launch = [&] {      // the kernel over a.rows: the plan, then the transposed plan
        with_vec(vec, [&](auto V) {
            with_act<GNNMP_ACT_SWISH>(job->act, [&](auto A) {
                megnet_edge_grad_kernel<decltype(V)::value, 4, decltype(A)::value><<<grid, 256, 0, (hipStream_t)stream>>>(a);
            });
        });
    };
    launch();
    GNNMP_LAUNCH_CHECK("megnet_edge_grad_kernel");
    if (!job->dQ) return GNNMP_OK;
    a.rows = plan_rows_whole(plan_t);      // the same heights: the same geometry and grid
    a.dz0 = nullptr;
    a.out = job->dQ;
    launch();
    GNNMP_LAUNCH_CHECK("megnet_edge_grad_kernel");
    return GNNMP_OK;
}

extern "C" int gnnmp_aggregate_grad_f32(const gnnmp_graph_t *plan, const gnnmp_aggregate_grad_t *job, int aggr, int64_t D,
                                        gnnmp_stream_t stream) {
    if (!plan) return fail(GNNMP_EINVAL, "aggregate_grad: null plan");
    if (!job) return fail(GNNMP_EINVAL, "aggregate_grad: null job");
    if (aggr != GNNMP_SUM && aggr != GNNMP_MEAN && aggr != GNNMP_MAX && aggr != GNNMP_MIN)
        return fail(GNNMP_EINVAL, "aggregate_grad: bad aggr %d", aggr);
    if (D < 1 || D > (1 << 19)) return fail(GNNMP_EINVAL, "aggregate_grad: bad D %lld", (long long)D);
    const bool sel = aggr == GNNMP_MAX || aggr == GNNMP_MIN;
    if (plan->n_total > 0) {      // no edge: nothing is read and no row of dm is written
        if (!job->dy) return fail(GNNMP_EINVAL, "aggregate_grad: null dy");
        if (!job->dm) return fail(GNNMP_EINVAL, "aggregate_grad: null dm");
        if (sel && !job->m) return fail(GNNMP_EINVAL, "aggregate_grad: null m (max / min need it)");
        if (sel && !job->y) return fail(GNNMP_EINVAL, "aggregate_grad: null y (max / min need it)");
    }
    GNNMP_TRY(check_edge_plan("aggregate_grad", plan, nullptr, false, "m has no row for them"));
    if (plan->n_dst == 0 || plan->n_total == 0) return GNNMP_OK;
    AggrGradArgs a = {};
    a.rows = plan_rows_whole(plan);
    a.dy = job->dy;
    a.m = sel ? job->m : nullptr;
    a.y = sel ? job->y : nullptr;
    a.acc = job->acc;
    a.dm = job->dm;
    a.D = (int)D;
    a.mean = aggr == GNNMP_MEAN;
    dim3 grid;
    const int vec = row_walk_geom("aggregate_grad", a.rows, D, 0, {a.dy, a.m, a.y, a.acc, a.dm}, a.geom, grid);
    if (vec < 0) return vec;
    const bool has_acc = job->acc != nullptr;
    with_vec(vec, [&](auto V) {
        constexpr int VEC = decltype(V)::value;
        if (sel && has_acc)
            aggregate_grad_kernel<VEC, 4, true, true><<<grid, 256, 0, (hipStream_t)stream>>>(a);
        else if (sel)
            aggregate_grad_kernel<VEC, 4, true, false><<<grid, 256, 0, (hipStream_t)stream>>>(a);
        else if (has_acc)
            aggregate_grad_kernel<VEC, 4, false, true><<<grid, 256, 0, (hipStream_t)stream>>>(a);
        else
            aggregate_grad_kernel<VEC, 4, false, false><<<grid, 256, 0, (hipStream_t)stream>>>(a);
    });
    GNNMP_LAUNCH_CHECK("aggregate_grad_kernel");
    return GNNMP_OK;
}
