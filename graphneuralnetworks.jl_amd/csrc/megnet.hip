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
// No atomics, no plan-owned scratch, every output element written exactly once (rows without in-edges and rows without out-edges
// included: zeros).  All three walk every row WHOLE, in plan order, whatever its length (PlanRows with n_chunks = 0, VROW_WHOLE), as
// cg_grad.hip does: every sum has the bits of the sequential fold, two calls give equal bits, and A HUB ROW IS WALKED BY ONE LANE
// GROUP: correct, slow.  Chunked hub rows are a later change.
//
// Registers: U = 4 slots in flight; per slot the edge kernel gathers two vectors, the pullback two, the aggregate pullback two — at most
// 32 VGPRs of loads with 16-byte lanes.  The compiler's resource report (LABNOTES.md) shows no scratch for any instance.
#include "csr_reduce.h"

namespace gnnmp {

struct MegnetEdgeArgs {
    PlanRows rows;               // the plan, n_chunks = 0 (rows are walked whole)
    RowGeom geom;
    const float *P, *Q;          // [n][hid]
    const float *F;              // [n_edges][hid], read by the HAS_F instances only
    float *a0;                   // [n_edges][hid]
    float *z0;                   // [n_edges][hid] or null
    int hid;
};

template <int VEC, int U, int ACT, bool HAS_F>
__global__ void __launch_bounds__(256) megnet_edge_kernel(const MegnetEdgeArgs a) {
    VRow vr;
    if (!decode_vrow<VROW_WHOLE>(a.rows, a.geom, blockIdx.x, vr)) return;
    const int row = vr.row, lig = vr.lig, gbase = vr.gbase, G = vr.G;
    const uint32_t beg = vr.beg, end = vr.end;
    const int f0 = ((int)blockIdx.y * G + lig) * VEC;
    const bool active = f0 < a.hid;      // inactive lanes of the last feature tile load nothing and store nothing
    const int64_t ld = a.hid;
    float pi[VEC];
#pragma unroll
    for (int q = 0; q < VEC; ++q) pi[q] = 0.0f;
    if (active) Vec<VEC>::load(a.P + (int64_t)row * ld + f0, pi);
    const bool store_z = a.z0 != nullptr;
    for (uint32_t base = beg; base < end; base += G) {   // slots are unsigned 32-bit (rowwalk.h)
        const uint32_t p = base + lig;
        int c = 0;
        uint32_t ev = 0;
        if (p < end) {
            c = a.rows.col[p];
            ev = (uint32_t)a.rows.eid[p];               // < n_edges: the export refuses a plan with self loops of its own
        }
        const int n = (int)min((uint32_t)G, end - base);
        for (int j = 0; j < n; j += U) {
            float qj[U][VEC], fe[HAS_F ? U : 1][VEC];
            int cjs[U];
            uint32_t ejs[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int jj = min(j + u, n - 1);
                cjs[u] = __shfl(c, gbase + jj, 64);
                ejs[u] = (uint32_t)__shfl((int)ev, gbase + jj, 64);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (active) {   // clamped, unconditional within the lane's activity (edge_conv.hip)
                    Vec<VEC>::load(a.Q + (int64_t)cjs[u] * ld + f0, qj[u]);
                    if (HAS_F) Vec<VEC>::load(a.F + (int64_t)ejs[u] * ld + f0, fe[HAS_F ? u : 0]);
                } else {
#pragma unroll
                    for (int q = 0; q < VEC; ++q) {
                        qj[u][q] = 0.0f;
                        if (HAS_F) fe[HAS_F ? u : 0][q] = 0.0f;
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (j + u < n && active) {
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
    PlanRows rows;               // pass 1: the plan; pass 2: the transposed plan.  n_chunks = 0
    RowGeom geom;
    const float *da0;            // [n_edges][hid]
    const float *z;              // [n_edges][hid]; not read by the IDENTITY instances
    float *dz0;                  // pass 1: [n_edges][hid] or null; pass 2: null
    float *out;                  // pass 1: dP [n][hid] or null; pass 2: dQ [n][hid]
    int hid;
};

template <int VEC, int U, int ACT>
__global__ void __launch_bounds__(256) megnet_edge_grad_kernel(const MegnetGradArgs a) {
    VRow vr;
    if (!decode_vrow<VROW_WHOLE>(a.rows, a.geom, blockIdx.x, vr)) return;
    const int row = vr.row, lig = vr.lig, gbase = vr.gbase, G = vr.G;
    const uint32_t beg = vr.beg, end = vr.end;
    const int f0 = ((int)blockIdx.y * G + lig) * VEC;
    const bool active = f0 < a.hid;
    const int64_t ld = a.hid;
    constexpr bool HAS_Z = ACT != GNNMP_ACT_IDENTITY;
    float acc[VEC];
#pragma unroll
    for (int q = 0; q < VEC; ++q) acc[q] = 0.0f;
    const bool store_e = a.dz0 != nullptr;
    for (uint32_t base = beg; base < end; base += G) {
        const uint32_t p = base + lig;
        uint32_t ev = 0;
        if (p < end) ev = (uint32_t)a.rows.eid[p];
        const int n = (int)min((uint32_t)G, end - base);
        for (int j = 0; j < n; j += U) {
            float da[U][VEC], zv[HAS_Z ? U : 1][VEC];
            uint32_t ejs[U];
#pragma unroll
            for (int u = 0; u < U; ++u) ejs[u] = (uint32_t)__shfl((int)ev, gbase + min(j + u, n - 1), 64);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (active) {
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
                if (j + u < n) {
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
    if (a.out != nullptr && active) Vec<VEC>::store(a.out + (int64_t)row * ld + f0, acc);
}

struct AggrGradArgs {
    PlanRows rows;               // the plan, n_chunks = 0
    RowGeom geom;
    const float *dy;             // [n_dst][D]
    const float *m, *y;          // [n_edges][D], [n_dst][D]: read by the SEL (max / min) instances only
    const float *acc;            // [n_edges][D], read by the HAS_ACC instances only
    float *dm;                   // [n_edges][D]
    int D, mean;
};

template <int VEC, int U, bool SEL, bool HAS_ACC>
__global__ void __launch_bounds__(256) aggregate_grad_kernel(const AggrGradArgs a) {
    VRow vr;
    if (!decode_vrow<VROW_WHOLE>(a.rows, a.geom, blockIdx.x, vr)) return;
    const int row = vr.row, lig = vr.lig, gbase = vr.gbase, G = vr.G;
    const uint32_t beg = vr.beg, end = vr.end;
    const int f0 = ((int)blockIdx.y * G + lig) * VEC;
    const bool active = f0 < a.D;
    const int64_t ld = a.D;
    float dv[VEC], yv[VEC];
#pragma unroll
    for (int q = 0; q < VEC; ++q) dv[q] = yv[q] = 0.0f;
    if (active && end > beg) {
        Vec<VEC>::load(a.dy + (int64_t)row * ld + f0, dv);
        if (SEL) Vec<VEC>::load(a.y + (int64_t)row * ld + f0, yv);
        if (a.mean) {            // divided once per row
            const float fdeg = (float)(end - beg);
#pragma unroll
            for (int q = 0; q < VEC; ++q) dv[q] = dv[q] / fdeg;
        }
    }
    for (uint32_t base = beg; base < end; base += G) {
        const uint32_t p = base + lig;
        uint32_t ev = 0;
        if (p < end) ev = (uint32_t)a.rows.eid[p];
        const int n = (int)min((uint32_t)G, end - base);
        for (int j = 0; j < n; j += U) {
            float mv[SEL ? U : 1][VEC], av[HAS_ACC ? U : 1][VEC];
            uint32_t ejs[U];
#pragma unroll
            for (int u = 0; u < U; ++u) ejs[u] = (uint32_t)__shfl((int)ev, gbase + min(j + u, n - 1), 64);
            if (SEL || HAS_ACC) {
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    if (active) {
                        if (SEL) Vec<VEC>::load(a.m + (int64_t)ejs[u] * ld + f0, mv[SEL ? u : 0]);
                        if (HAS_ACC) Vec<VEC>::load(a.acc + (int64_t)ejs[u] * ld + f0, av[HAS_ACC ? u : 0]);
                    } else {
#pragma unroll
                        for (int q = 0; q < VEC; ++q) {
                            if (SEL) mv[SEL ? u : 0][q] = 0.0f;
                            if (HAS_ACC) av[HAS_ACC ? u : 0][q] = 0.0f;
                        }
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (j + u < n && active) {
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

static PlanRows megnet_whole_rows(const gnnmp_graph_t *plan) {
    PlanRows r = plan_rows(plan);
    r.n_chunks = 0;     // no chunk virtual rows: VROW_WHOLE walks the long rows themselves
    r.n_long = 0;
    return r;
}

// the vector width every array of the call admits and the row walk's geometry for it; < 0: refused
static int megnet_geom(const char *who, const PlanRows &rows, RowGeom &geom, int64_t D, std::initializer_list<const float *> ptrs, dim3 &grid) {
    uintptr_t align = 0;
    for (const float *p : ptrs) align |= reinterpret_cast<uintptr_t>(p);
    const int vec = pick_vec(D, reinterpret_cast<const void *>(align), nullptr);
    geom = RowGeom{pick_log2g((D + vec - 1) / vec), 4, 0, 0};
    if (row_blocks(rows, geom) >= INT32_MAX) return fail(GNNMP_EUNSUPPORTED, "%s: too many row blocks", who);
    grid = row_grid(rows, geom, feature_tiles(D, vec, geom.log2g));
    return vec;
}

template <class F>
static void with_megnet_act(int act, F &&f) {
    switch (act) {
        case GNNMP_ACT_RELU: return f(int_c<GNNMP_ACT_RELU>{});
        case GNNMP_ACT_SOFTPLUS: return f(int_c<GNNMP_ACT_SOFTPLUS>{});
        case GNNMP_ACT_TANH: return f(int_c<GNNMP_ACT_TANH>{});
        case GNNMP_ACT_SWISH: return f(int_c<GNNMP_ACT_SWISH>{});
        default: return f(int_c<GNNMP_ACT_IDENTITY>{});
    }
}

// what the two MEGNet exports ask of their plans
static int megnet_check_plan(const char *who, const gnnmp_graph_t *plan, const gnnmp_graph_t *plan_t) {
    if (plan->n_src != plan->n_dst)
        return fail(GNNMP_EINVAL, "%s: the plan is not square (%lld sources, %lld destinations)", who, (long long)plan->n_src,
                    (long long)plan->n_dst);
    if (plan_t) {
        if (plan_t->n_dst != plan->n_dst || plan_t->n_src != plan->n_src)
            return fail(GNNMP_EINVAL, "%s: the transposed plan has %lld rows, the plan %lld", who, (long long)plan_t->n_dst,
                        (long long)plan->n_dst);
        if (plan_t->n_edges != plan->n_edges || plan_t->n_total != plan->n_total)
            return fail(GNNMP_EINVAL, "%s: the transposed plan has %lld edges, the plan %lld", who, (long long)plan_t->n_total,
                        (long long)plan->n_total);
    }
    if (plan->n_total != plan->n_edges)
        return fail(GNNMP_EINVAL, "%s: the plan was built with self loops (%lld slots, %lld edges): the E-row arrays have no row for them",
                    who, (long long)plan->n_total, (long long)plan->n_edges);
    return GNNMP_OK;
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
    GNNMP_TRY(megnet_check_plan("megnet_edge", plan, nullptr));
    if (plan->n_dst == 0 || plan->n_total == 0) return GNNMP_OK;
    MegnetEdgeArgs a = {};
    a.rows = megnet_whole_rows(plan);
    a.P = job->P;
    a.Q = job->Q;
    a.F = job->F;
    a.a0 = job->a0;
    a.z0 = job->z0;
    a.hid = (int)hid;
    dim3 grid;
    const int vec = megnet_geom("megnet_edge", a.rows, a.geom, hid, {job->P, job->Q, job->F, job->a0, job->z0}, grid);
    if (vec < 0) return vec;
    const bool has_f = job->F != nullptr;
    with_vec(vec, [&](auto V) {
        with_megnet_act(job->act, [&](auto A) {
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
    GNNMP_TRY(megnet_check_plan("megnet_edge_grad", plan, job->dQ ? plan_t : nullptr));
    if (plan->n_dst == 0) return GNNMP_OK;
    if (plan->n_total == 0 && !job->dP) return GNNMP_OK;
    MegnetGradArgs a = {};
    a.rows = megnet_whole_rows(plan);
    a.da0 = job->da0;
    a.z = job->act != GNNMP_ACT_IDENTITY ? job->z : nullptr;
    a.dz0 = plan->n_total > 0 ? job->dz0 : nullptr;
    a.out = job->dP;
    a.hid = (int)hid;
    dim3 grid;
    const int vec = megnet_geom("megnet_edge_grad", a.rows, a.geom, hid, {a.da0, a.z, job->dz0, job->dP, job->dQ}, grid);
    if (vec < 0) return vec;
    with_vec(vec, [&](auto V) {
        with_megnet_act(job->act, [&](auto A) {
            megnet_edge_grad_kernel<decltype(V)::value, 4, decltype(A)::value><<<grid, 256, 0, (hipStream_t)stream>>>(a);
        });
    });
    GNNMP_LAUNCH_CHECK("megnet_edge_grad_kernel");
    if (!job->dQ) return GNNMP_OK;
    a.rows = megnet_whole_rows(plan_t);      // the same heights: the same geometry and grid
    a.dz0 = nullptr;
    a.out = job->dQ;
    with_vec(vec, [&](auto V) {
        with_megnet_act(job->act, [&](auto A) {
            megnet_edge_grad_kernel<decltype(V)::value, 4, decltype(A)::value><<<grid, 256, 0, (hipStream_t)stream>>>(a);
        });
    });
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
    if (plan->n_total != plan->n_edges)
        return fail(GNNMP_EINVAL, "aggregate_grad: the plan was built with self loops (%lld slots, %lld edges): m has no row for them",
                    (long long)plan->n_total, (long long)plan->n_edges);
    if (plan->n_dst == 0 || plan->n_total == 0) return GNNMP_OK;
    AggrGradArgs a = {};
    a.rows = megnet_whole_rows(plan);
    a.dy = job->dy;
    a.m = sel ? job->m : nullptr;
    a.y = sel ? job->y : nullptr;
    a.acc = job->acc;
    a.dm = job->dm;
    a.D = (int)D;
    a.mean = aggr == GNNMP_MEAN;
    dim3 grid;
    const int vec = megnet_geom("aggregate_grad", a.rows, a.geom, D, {a.dy, a.m, a.y, a.acc, a.dm}, grid);
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
