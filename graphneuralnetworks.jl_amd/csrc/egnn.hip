// egnn.hip — the edge and coordinate steps of EGNNConv (egnn_conv, GNNlib/src/layers/conv.jl:459-495), forward and pullback, without a
// single [E][Dx] array.  Edge k: j -> i; W0 = [A | B | c | D] is ϕe's first weight; P = h A' + b0, Q = h B' [N][hid] and F = e D' [E][hid]
// come from the caller's dense calls (include/gnnmp.h states the arithmetic):
//     d_k = x_i − x_j     q_k = Σ_a d_k[a]²  (a ascending from 0, products rounded then added)     r_k = sqrt(q_k)     n_k = d_k / (r_k + 1e-6)
//   egnn_edge_kernel        K1, original edge order: q, z0_k = ((P_i + Q_j) + q_k c) (+ F_k), a0 = act(z0) by bias_act_apply — the device
//                           function of gnnmp_bias_act_f32.  A lane group takes one edge and VEC features a lane; every lane of the group
//                           computes q_k itself (2 Dx broadcast loads), the first lane of the first feature tile stores it.
//   egnn_coord_kernel       K2: a lane group owns destination i and holds x_i in registers; its lanes run over the row's EDGES, each lane
//                           gathers x_j, reads mx[eid], recomputes n_k; x'_i = x_i + (Σ mx_k n_k) / deg_i (deg_i = 0: x'_i = x_i).
//   egnn_coord_grad_kernel  K3, the same row shape: the in-edges of i from the plan (dmx[eid] = (n_k · Δx'_i) / deg_i, and the in-part of
//                           dx_i), then — for dx — the out-edges of i from the transposed plan, which gather x, Δx' and the in-degree of
//                           the edge's destination, mx[eid] and dq[eid]:
//                               g_k = (mx_k / deg_i) Δx'_i      dd_k = (g_k / den − d_k ((d_k · g_k) / (r_k den²))) + (2 dq_k) d_k,  den = r_k + 1e-6
//                               dx_i = (Δx'_i + Σ_{k into i} dd_k) − Σ_{k out of i} dd_k
//                           q_k == 0 (a self loop, coincident points): the n-path terms are DEFINED as 0 (dd_k = 2 dq_k d_k = 0, dmx_k = 0
//                           comes out by itself); the reference's AD gives Inf * 0 there.
//   act_grad_z_kernel       dz = dy ⊙ act'(z) from the pre-activation, all five gnnmp_act codes
// K2 / K3 are whole-row walks on the conventions of slotwalk.h (a hub row by one lane group); their lanes stride over the edges themselves,
// so of the shared pieces they take only group_sum.  Summation order of a row: G lanes, G = the smallest power of two >= the plan's mean row length (<= 64); lane l
// folds slots l, l + G, ... sequentially from 0, then a butterfly p[l] + p[l ^ m], m = G/2 .. 1.  It depends on the plan only: either
// output of K3 has the same bits whether or not the other is asked for, and two calls give equal bits.
//
// Registers: a node's Dx <= 16 coordinates live in registers, so the kernels are instantiated for the capacities DXC = 1, 2, 3, 4, 8, 16
// (the smallest one that holds Dx; components beyond Dx are zeros and add exact zeros to q_k).  The compiler's resource report
// (LABNOTES.md) shows no scratch for any instance.
#include "csr_reduce.h"
#include "launch.h"

namespace gnnmp {

constexpr float EGNN_EPS = 1e-6f;

// ---- K1 ---------------------------------------------------------------------------------------------------------------------------
struct EgnnEdgeArgs {
    const void *s, *t;
    int idx_bytes, index_base;
    const float *x, *P, *Q, *F, *c;
    float *q, *a0, *z0;
    int64_t E;
    int hid, Dx, log2g;
};

template <int VEC, int ACT, bool HAS_F>
__global__ void __launch_bounds__(256) egnn_edge_kernel(const EgnnEdgeArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int G = 1 << a.log2g;
    const int lig = lane & (G - 1);
    const int64_t k = (((int64_t)blockIdx.x * 4 + wave) << (6 - a.log2g)) + (lane >> a.log2g);
    if (k >= a.E) return;
    const int64_t i = load_index(a.t, k, a.idx_bytes, a.index_base), j = load_index(a.s, k, a.idx_bytes, a.index_base);
    const float *xi = a.x + i * a.Dx, *xj = a.x + j * a.Dx;
    float q = 0.0f;
    for (int c = 0; c < a.Dx; ++c) {
        const float d = xi[c] - xj[c];
        q = q + d * d;
    }
    if (blockIdx.y == 0 && lig == 0) a.q[k] = q;
    const int f0 = ((int)blockIdx.y * G + lig) * VEC;
    if (f0 >= a.hid) return;      // inactive lanes of the last feature tile
    float p[VEC], qj[VEC], cv[VEC], z[VEC], y[VEC];
    Vec<VEC>::load(a.P + i * a.hid + f0, p);
    Vec<VEC>::load(a.Q + j * a.hid + f0, qj);
    Vec<VEC>::load(a.c + f0, cv);
#pragma unroll
    for (int v = 0; v < VEC; ++v) z[v] = (p[v] + qj[v]) + q * cv[v];
    if (HAS_F) {
        float f[VEC];
        Vec<VEC>::load(a.F + k * a.hid + f0, f);
#pragma unroll
        for (int v = 0; v < VEC; ++v) z[v] = z[v] + f[v];
    }
    if (a.z0) Vec<VEC>::store(a.z0 + k * a.hid + f0, z);
#pragma unroll
    for (int v = 0; v < VEC; ++v) y[v] = bias_act_apply(z[v], ACT);
    Vec<VEC>::store(a.a0 + k * a.hid + f0, y);
}

// ---- K2 / K3 ----------------------------------------------------------------------------------------------------------------------
template <int DXC>
__device__ __forceinline__ void load_coord(const float *p, int Dx, float v[DXC]) {
#pragma unroll
    for (int c = 0; c < DXC; ++c) v[c] = c < Dx ? p[c] : 0.0f;
}

// d = xi − xj, q = Σ d², r = sqrt(q)
template <int DXC>
__device__ __forceinline__ void egnn_pair(const float xi[DXC], const float xj[DXC], float d[DXC], float &q, float &r) {
    q = 0.0f;
#pragma unroll
    for (int c = 0; c < DXC; ++c) {
        d[c] = xi[c] - xj[c];
        q = q + d[c] * d[c];
    }
    r = sqrtf(q);
}

// acc += dd_k, from d_k, q_k, r_k, s = mx_k / deg_i, Δx'_i and dq_k
template <int DXC>
__device__ __forceinline__ void egnn_add_dd(const float d[DXC], float q, float r, float s, const float dl[DXC], float dq, float acc[DXC]) {
    const float two_dq = 2.0f * dq;
    if (q > 0.0f) {
        const float den = r + EGNN_EPS;
        float g[DXC], dg = 0.0f;
#pragma unroll
        for (int c = 0; c < DXC; ++c) {
            g[c] = s * dl[c];
            dg = dg + d[c] * g[c];
        }
        const float coef = dg / (r * (den * den));
#pragma unroll
        for (int c = 0; c < DXC; ++c) acc[c] = acc[c] + ((g[c] / den - d[c] * coef) + two_dq * d[c]);
    } else {      // the n-path terms are defined as 0 (d is 0 here, so is the rest)
#pragma unroll
        for (int c = 0; c < DXC; ++c) acc[c] = acc[c] + two_dq * d[c];
    }
}

struct EgnnCoordArgs {
    PlanRows rows;      // whole rows (plan_rows_whole)
    RowGeom geom;
    const float *x, *mx;
    float *xo;
    int Dx;
};

template <int DXC>
__global__ void __launch_bounds__(256) egnn_coord_kernel(const EgnnCoordArgs a) {
    VRow vr;
    if (!decode_vrow<VROW_WHOLE>(a.rows, a.geom, blockIdx.x, vr)) return;
    const int row = vr.row, lig = vr.lig, G = vr.G;
    const uint32_t beg = vr.beg, end = vr.end;
    float xi[DXC], acc[DXC];
    load_coord<DXC>(a.x + (int64_t)row * a.Dx, a.Dx, xi);
#pragma unroll
    for (int c = 0; c < DXC; ++c) acc[c] = 0.0f;
    for (uint32_t p = beg + lig; p < end; p += G) {      // slots are unsigned 32-bit with headroom (rowwalk.h): p + G cannot wrap
        const int j = a.rows.col[p];
        const uint32_t ev = (uint32_t)a.rows.eid[p];     // < n_edges: the export refuses a plan with self loops of its own
        float xj[DXC], d[DXC], q, r;
        load_coord<DXC>(a.x + (int64_t)j * a.Dx, a.Dx, xj);
        egnn_pair<DXC>(xi, xj, d, q, r);
        const float m = a.mx[ev], den = r + EGNN_EPS;
#pragma unroll
        for (int c = 0; c < DXC; ++c) acc[c] = acc[c] + m * (d[c] / den);
    }
    group_sum<DXC>(acc, G);
    if (lig == 0) {
        const uint32_t deg = end - beg;
        const float fdeg = (float)deg;
#pragma unroll
        for (int c = 0; c < DXC; ++c) {
            if (c < a.Dx) a.xo[(int64_t)row * a.Dx + c] = deg ? xi[c] + acc[c] / fdeg : xi[c];
        }
    }
}

struct EgnnCoordGradArgs {
    PlanRows rows;          // the plan, whole rows
    const uint32_t *t_rowptr;   // the transposed plan: row j lists the edges that leave j
    const int32_t *t_col, *t_eid;
    RowGeom geom;
    const float *x, *dxo, *mx, *dq;
    float *dmx, *dx;
    int Dx;
};

template <int DXC, bool WANT_DMX, bool WANT_DX>
__global__ void __launch_bounds__(256) egnn_coord_grad_kernel(const EgnnCoordGradArgs a) {
    VRow vr;
    if (!decode_vrow<VROW_WHOLE>(a.rows, a.geom, blockIdx.x, vr)) return;
    const int row = vr.row, lig = vr.lig, G = vr.G;
    const uint32_t beg = vr.beg, end = vr.end;
    const float fdeg = (float)(end - beg);
    float xi[DXC], di[DXC], acc_in[DXC];
    load_coord<DXC>(a.x + (int64_t)row * a.Dx, a.Dx, xi);
    load_coord<DXC>(a.dxo + (int64_t)row * a.Dx, a.Dx, di);
#pragma unroll
    for (int c = 0; c < DXC; ++c) acc_in[c] = 0.0f;
    for (uint32_t p = beg + lig; p < end; p += G) {      // the edges into `row`
        const int j = a.rows.col[p];
        const uint32_t ev = (uint32_t)a.rows.eid[p];
        float xj[DXC], d[DXC], q, r;
        load_coord<DXC>(a.x + (int64_t)j * a.Dx, a.Dx, xj);
        egnn_pair<DXC>(xi, xj, d, q, r);
        if (WANT_DMX) {
            const float den = r + EGNN_EPS;
            float dot = 0.0f;
#pragma unroll
            for (int c = 0; c < DXC; ++c) dot = dot + (d[c] / den) * di[c];
            a.dmx[ev] = dot / fdeg;
        }
        if (WANT_DX) egnn_add_dd<DXC>(d, q, r, a.mx[ev] / fdeg, di, a.dq[ev], acc_in);
    }
    if (!WANT_DX) return;
    float acc_out[DXC];
#pragma unroll
    for (int c = 0; c < DXC; ++c) acc_out[c] = 0.0f;
    const uint32_t tbeg = a.t_rowptr[row], tend = a.t_rowptr[row + 1];
    for (uint32_t p = tbeg + lig; p < tend; p += G) {    // the edges out of `row`: row -> i
        const int i = a.t_col[p];
        const uint32_t ev = (uint32_t)a.t_eid[p];
        float xd[DXC], dl[DXC], d[DXC], q, r;
        load_coord<DXC>(a.x + (int64_t)i * a.Dx, a.Dx, xd);
        load_coord<DXC>(a.dxo + (int64_t)i * a.Dx, a.Dx, dl);
        const float fdi = (float)(a.rows.rowptr[i + 1] - a.rows.rowptr[i]);     // >= 1: this edge enters i
        egnn_pair<DXC>(xd, xi, d, q, r);
        egnn_add_dd<DXC>(d, q, r, a.mx[ev] / fdi, dl, a.dq[ev], acc_out);
    }
    group_sum<DXC>(acc_in, G);
    group_sum<DXC>(acc_out, G);
    if (lig == 0) {
#pragma unroll
        for (int c = 0; c < DXC; ++c) {
            if (c < a.Dx) a.dx[(int64_t)row * a.Dx + c] = (di[c] + acc_in[c]) - acc_out[c];
        }
    }
}

// ---- act'(z) ------------------------------------------------------------------------------------------------------------------------
// act_dz of csr_reduce.h (hardware transcendentals, the formulas of cg_grad.hip), shared with megnet.hip
// thread i takes elements [i VEC, i VEC + VEC); the last thread of a VEC > 1 launch finishes the tail element by element
template <int VEC, int ACT>
__global__ void __launch_bounds__(256) act_grad_z_kernel(const float *dy, const float *z, float *dz, int64_t n) {
    const int64_t e0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * VEC;
    if (e0 >= n) return;
    if (e0 + VEC <= n) {
        float d[VEC], zv[VEC], o[VEC];
        Vec<VEC>::load(dy + e0, d);
        if (ACT != GNNMP_ACT_IDENTITY) Vec<VEC>::load(z + e0, zv);
#pragma unroll
        for (int v = 0; v < VEC; ++v) o[v] = act_dz<ACT>(d[v], ACT != GNNMP_ACT_IDENTITY ? zv[v] : 0.0f);
        Vec<VEC>::store(dz + e0, o);
    } else {
        for (int64_t e = e0; e < n; ++e) dz[e] = act_dz<ACT>(dy[e], ACT != GNNMP_ACT_IDENTITY ? z[e] : 0.0f);
    }
}

// the register capacity that holds Dx coordinates
template <class F>
static void with_dxc(int Dx, F &&f) {
    if (Dx <= 1) return f(int_c<1>{});
    if (Dx == 2) return f(int_c<2>{});
    if (Dx == 3) return f(int_c<3>{});
    if (Dx == 4) return f(int_c<4>{});
    if (Dx <= 8) return f(int_c<8>{});
    return f(int_c<16>{});
}

// lanes per row: the smallest power of two >= the plan's mean row length
static RowGeom egnn_row_geom(const gnnmp_graph_t *plan) {
    const int64_t mean = plan->n_dst > 0 ? (plan->n_total + plan->n_dst - 1) / plan->n_dst : 1;
    return RowGeom{pick_log2g(mean), 4, 0, 0};
}

}  // namespace gnnmp

using namespace gnnmp;

extern "C" int gnnmp_egnn_edge_f32(const gnnmp_egnn_edge_t *job, int64_t E, int64_t hid, int64_t Dx, gnnmp_stream_t stream) {
    if (!job) return fail(GNNMP_EINVAL, "egnn_edge: null job");
    if (!job->s) return fail(GNNMP_EINVAL, "egnn_edge: null s");
    if (!job->t) return fail(GNNMP_EINVAL, "egnn_edge: null t");
    if (!job->x) return fail(GNNMP_EINVAL, "egnn_edge: null x");
    if (!job->P) return fail(GNNMP_EINVAL, "egnn_edge: null P");
    if (!job->Q) return fail(GNNMP_EINVAL, "egnn_edge: null Q");
    if (!job->c) return fail(GNNMP_EINVAL, "egnn_edge: null c");
    if (!job->q) return fail(GNNMP_EINVAL, "egnn_edge: null q");
    if (!job->a0) return fail(GNNMP_EINVAL, "egnn_edge: null a0");
    if (job->idx_bytes != 4 && job->idx_bytes != 8) return fail(GNNMP_EINVAL, "egnn_edge: bad idx_bytes %d", job->idx_bytes);
    if (E < 0) return fail(GNNMP_EINVAL, "egnn_edge: negative E");
    if (hid < 1 || hid > (1 << 19)) return fail(GNNMP_EINVAL, "egnn_edge: bad hid %lld", (long long)hid);
    if (Dx < 1 || Dx > 16) return fail(GNNMP_EINVAL, "egnn_edge: bad Dx %lld", (long long)Dx);
    if (job->act < GNNMP_ACT_IDENTITY || job->act > GNNMP_ACT_SWISH) return fail(GNNMP_EINVAL, "egnn_edge: bad act %d", job->act);
    if (E == 0) return GNNMP_OK;
    EgnnEdgeArgs a = {};
    a.s = job->s;
    a.t = job->t;
    a.idx_bytes = job->idx_bytes;
    a.index_base = job->index_base;
    a.x = job->x;
    a.P = job->P;
    a.Q = job->Q;
    a.F = job->F;
    a.c = job->c;
    a.q = job->q;
    a.a0 = job->a0;
    a.z0 = job->z0;
    a.E = E;
    a.hid = (int)hid;
    a.Dx = (int)Dx;
    uintptr_t align = 0;
    const float *const ptrs[] = {job->P, job->Q, job->F, job->c, job->a0, job->z0};
    for (const float *p : ptrs) align |= reinterpret_cast<uintptr_t>(p);
    const int vec = pick_vec(hid, reinterpret_cast<const void *>(align), nullptr);
    a.log2g = pick_log2g((hid + vec - 1) / vec);
    const int64_t per_block = (int64_t)4 << (6 - a.log2g);
    const int64_t blocks = (E + per_block - 1) / per_block;
    if (blocks >= INT32_MAX) return fail(GNNMP_EUNSUPPORTED, "egnn_edge: too many edge blocks");
    const dim3 grid((unsigned)blocks, (unsigned)feature_tiles(hid, vec, a.log2g));
    const bool has_f = job->F != nullptr;
    with_vec(vec, [&](auto V) {
        with_act<GNNMP_ACT_SWISH>(job->act, [&](auto A) {
            if (has_f)
                egnn_edge_kernel<decltype(V)::value, decltype(A)::value, true><<<grid, 256, 0, (hipStream_t)stream>>>(a);
            else
                egnn_edge_kernel<decltype(V)::value, decltype(A)::value, false><<<grid, 256, 0, (hipStream_t)stream>>>(a);
        });
    });
    GNNMP_LAUNCH_CHECK("egnn_edge_kernel");
    return GNNMP_OK;
}

extern "C" int gnnmp_egnn_coord_f32(const gnnmp_graph_t *plan, const gnnmp_egnn_coord_t *job, int64_t Dx, gnnmp_stream_t stream) {
    if (!plan) return fail(GNNMP_EINVAL, "egnn_coord: null plan");
    if (!job) return fail(GNNMP_EINVAL, "egnn_coord: null job");
    if (!job->x) return fail(GNNMP_EINVAL, "egnn_coord: null x");
    if (!job->mx && plan->n_total > 0) return fail(GNNMP_EINVAL, "egnn_coord: null mx");      // no edge: no entry of mx is read
    if (!job->xo) return fail(GNNMP_EINVAL, "egnn_coord: null xo");
    if (Dx < 1 || Dx > 16) return fail(GNNMP_EINVAL, "egnn_coord: bad Dx %lld", (long long)Dx);
    GNNMP_TRY(check_edge_plan("egnn_coord", plan, nullptr, true, "mx has no entry for them"));
    if (plan->n_dst == 0) return GNNMP_OK;
    EgnnCoordArgs a = {};
    a.rows = plan_rows_whole(plan);
    a.geom = egnn_row_geom(plan);
    a.x = job->x;
    a.mx = job->mx;
    a.xo = job->xo;
    a.Dx = (int)Dx;
    dim3 grid;
    GNNMP_TRY(row_walk_grid("egnn_coord", a.rows, a.geom, 1, grid));
    with_dxc(a.Dx, [&](auto C) { egnn_coord_kernel<decltype(C)::value><<<grid, 256, 0, (hipStream_t)stream>>>(a); });
    GNNMP_LAUNCH_CHECK("egnn_coord_kernel");
    return GNNMP_OK;
}

extern "C" int gnnmp_egnn_coord_grad_f32(const gnnmp_graph_t *plan, const gnnmp_graph_t *plan_t, const gnnmp_egnn_coord_grad_t *job,
                                         int64_t Dx, gnnmp_stream_t stream) {
    if (!plan) return fail(GNNMP_EINVAL, "egnn_coord_grad: null plan");
    if (!job) return fail(GNNMP_EINVAL, "egnn_coord_grad: null job");
    if (!job->x) return fail(GNNMP_EINVAL, "egnn_coord_grad: null x");
    if (!job->dxo) return fail(GNNMP_EINVAL, "egnn_coord_grad: null dxo");
    if (!job->dmx && !job->dx) return fail(GNNMP_EINVAL, "egnn_coord_grad: dmx and dx are both null");
    if (job->dx && !plan_t) return fail(GNNMP_EINVAL, "egnn_coord_grad: dx without plan_t");
    if (job->dx && !job->mx && plan->n_total > 0) return fail(GNNMP_EINVAL, "egnn_coord_grad: dx without mx");      // no edge: not read
    if (job->dx && !job->dq && plan->n_total > 0) return fail(GNNMP_EINVAL, "egnn_coord_grad: dx without dq");
    if (Dx < 1 || Dx > 16) return fail(GNNMP_EINVAL, "egnn_coord_grad: bad Dx %lld", (long long)Dx);
    GNNMP_TRY(check_edge_plan("egnn_coord_grad", plan, plan_t, true, "mx has no entry for them"));
    if (plan->n_dst == 0) return GNNMP_OK;
    EgnnCoordGradArgs a = {};
    a.rows = plan_rows_whole(plan);
    a.geom = egnn_row_geom(plan);
    if (job->dx) {
        a.t_rowptr = plan_t->rowptr;
        a.t_col = plan_t->col;
        a.t_eid = plan_t->eid;
    }
    a.x = job->x;
    a.dxo = job->dxo;
    a.mx = job->mx;
    a.dq = job->dq;
    a.dmx = job->dmx;
    a.dx = job->dx;
    a.Dx = (int)Dx;
    dim3 grid;
    GNNMP_TRY(row_walk_grid("egnn_coord_grad", a.rows, a.geom, 1, grid));
    const bool want_dmx = job->dmx != nullptr, want_dx = job->dx != nullptr;
    with_dxc(a.Dx, [&](auto C) {
        constexpr int DXC = decltype(C)::value;
        if (want_dmx && want_dx)
            egnn_coord_grad_kernel<DXC, true, true><<<grid, 256, 0, (hipStream_t)stream>>>(a);
        else if (want_dx)
            egnn_coord_grad_kernel<DXC, false, true><<<grid, 256, 0, (hipStream_t)stream>>>(a);
        else
            egnn_coord_grad_kernel<DXC, true, false><<<grid, 256, 0, (hipStream_t)stream>>>(a);
    });
    GNNMP_LAUNCH_CHECK("egnn_coord_grad_kernel");
    return GNNMP_OK;
}

extern "C" int gnnmp_act_grad_z_f32(const gnnmp_act_grad_z_t *job, int64_t n, gnnmp_stream_t stream) {
    if (!job) return fail(GNNMP_EINVAL, "act_grad_z: null job");
    if (n < 0) return fail(GNNMP_EINVAL, "act_grad_z: negative n");
    if (job->act < GNNMP_ACT_IDENTITY || job->act > GNNMP_ACT_SWISH) return fail(GNNMP_EINVAL, "act_grad_z: bad act %d", job->act);
    if (!job->dy) return fail(GNNMP_EINVAL, "act_grad_z: null dy");
    if (!job->dz) return fail(GNNMP_EINVAL, "act_grad_z: null dz");
    if (job->act != GNNMP_ACT_IDENTITY && !job->z) return fail(GNNMP_EINVAL, "act_grad_z: null z");
    if (n == 0) return GNNMP_OK;
    const int vec = narrow_vec(4, job->dy, job->z, job->dz) == 4 ? 4 : 1;
    const int64_t threads = (n + vec - 1) / vec;
    const int64_t blocks = (threads + 255) / 256;
    if (blocks >= INT32_MAX) return fail(GNNMP_EUNSUPPORTED, "act_grad_z: too many blocks");
    const float *dy = job->dy, *z = job->z;
    float *dz = job->dz;
    with_act<GNNMP_ACT_SWISH>(job->act, [&](auto A) {
        if (vec == 4)
            act_grad_z_kernel<4, decltype(A)::value><<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(dy, z, dz, n);
        else
            act_grad_z_kernel<1, decltype(A)::value><<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(dy, z, dz, n);
    });
    GNNMP_LAUNCH_CHECK("act_grad_z_kernel");
    return GNNMP_OK;
}
