// nn_grad.hip — the pullback of nn_conv's per-edge-matrix message (nn_conv, GNNlib/src/layers/conv.jl:260-273), as ONE walk of the
// transposed plan.  The forward (gnnmp_propagate_nn_f32, nn_rows_kernel of propagate.hip) reads one (Dout, Din) matrix per edge,
// W_k = reshape(nn(e_k), Dout, Din) — `we` [E][Dout * Din], element (o, c) of edge k at we[k][o + Dout * c] — and forms
// m_i = Σ_{k: j -> i} W_k x_j.  Given Δ [N][Dout] at the DESTINATIONS, for edge k: j -> i at original position k
//     dwe[k][o + Dout * c] = Δ[i][o] * x[j][c]                              (E * Dout * Din values: the gradient arriving at nn(e))
//     dx[j][c]             = Σ_{k out of j} Σ_o we[k][o + Dout * c] * Δ[i][o]
// `we` and `dwe` are E * Dout * Din * 4 bytes each (16 KB an edge at 64 x 64); everything else of the layer is N rows.  So the walk reads
// we once, writes dwe once, and moves nothing else of that size: a lane group owns SOURCE j (row j of the transposed plan: the edges
// that leave j, col = the destination, eid = the original position), x_j is the row's own, and for each edge the group gathers Δ_i,
// reads W_k, stores dW_k and accumulates dx_j.  Every edge lies in exactly one row of the transposed plan: no atomics, no scratch, every
// output element written exactly once (rows without out-edges: zeros), two calls give equal bits.
//
// Geometry.  Lane `lig` of the group owns the outputs o = (t G + lig) VEC + q, q < VEC, t = 0, 1, ... (G lanes a group, VEC floats a
// lane): for one in-channel c the Dout weights of an edge are one contiguous run, so every we / dwe access of a group is coalesced; a
// lane loops over t when Dout > G * VEC.  A workgroup handles a tile of TC = 8 in-channels (blockIdx.y): the tile's TC * Dout weights of
// an edge are contiguous too (2 KB at Dout = 64).  Each lane keeps ONE partial of dx_j[c] per channel of the tile in registers across
// ALL edges of the row and the group reduces them once per row — TC * log2(G) shuffles a row, not per edge.  U edges are in flight at a
// time (U * TC loads of we and U of Δ are issued before the first product: nn_rows_kernel measured a third of the HBM rate with one
// edge in flight); U = 4 with 4- and 8-byte lanes, 2 with 16-byte lanes (64 VGPRs of weights either way).
//
// Summation order of dx[j][c] (the float32 restatement of tests/nn_conv_ref.py follows it): products are rounded, then added
// (-ffp-contract=off).  A lane folds its own products sequentially — edges in row order in batches of U; inside a batch output tile t
// ascending, then the edges of the batch, then q ascending — from 0.0f; lanes that own no output hold 0.0f.  The G lane partials are
// then summed by a butterfly: for m = G / 2, G / 4, ..., 1: p[lane] = p[lane] + p[lane ^ m].
//
// A whole-row walk on the conventions of slotwalk.h (a hub row by one lane group); its lanes stride over the edges themselves, so of the
// shared pieces it takes only group_sum.
// The compiler's resource report (LABNOTES.md) shows no scratch for any instance.
#include "csr_reduce.h"
#include "launch.h"

namespace gnnmp {

struct NnGradArgs {
    PlanRows rows;       // the TRANSPOSED plan, whole rows (plan_rows_whole)
    RowGeom geom;
    const float *x;      // [n][Din]
    const float *we;     // [n_edges][Dout * Din], read by the WANT_DX instances only
    const float *dm;     // [n][Dout]
    float *dx;           // [n][Din], WANT_DX
    float *dwe;          // [n_edges][Dout * Din], WANT_DW
    int Din, Dout;
};

constexpr int NN_GRAD_TC = 8;      // in-channels a workgroup handles

template <int VEC, int U, bool WANT_DX, bool WANT_DW>
__global__ void __launch_bounds__(256) nn_grad_rows_kernel(const NnGradArgs a) {
    constexpr int TC = NN_GRAD_TC;
    VRow vr;
    if (!decode_vrow<VROW_WHOLE>(a.rows, a.geom, blockIdx.x, vr)) return;
    const int row = vr.row, lig = vr.lig, G = vr.G;
    const uint32_t beg = vr.beg, end = vr.end;
    const int c0 = (int)blockIdx.y * TC;
    const int nc = min(TC, a.Din - c0);      // >= 1: grid.y covers Din
    const int Dout = a.Dout;
    const int64_t slab = (int64_t)Dout * a.Din;
    float xj[TC], acc[TC];
#pragma unroll
    for (int c = 0; c < TC; ++c) {
        xj[c] = a.x[(int64_t)row * a.Din + c0 + min(c, nc - 1)];   // channels past the tile's end re-read its last one and are never used
        acc[c] = 0.0f;
    }
    // U edges at a time; slots past the end re-read the last edge and are neither folded nor stored
    for (uint32_t p0 = beg; p0 < end; p0 += U) {
        int64_t di[U], eo[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t p = min(p0 + u, end - 1);
            di[u] = (int64_t)a.rows.col[p] * Dout;                                      // the destination's row of Δ
            eo[u] = (int64_t)(uint32_t)a.rows.eid[p] * slab + (int64_t)c0 * Dout;      // < n_edges: the export refuses plan-added self loops
        }
        for (int o = lig * VEC; o < Dout; o += G * VEC) {
            float d[U][VEC], w[WANT_DX ? U : 1][TC][VEC];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                Vec<VEC>::load(a.dm + di[u] + o, d[u]);
                if (WANT_DX) {
#pragma unroll
                    for (int c = 0; c < TC; ++c)
                        Vec<VEC>::load(a.we + eo[u] + (int64_t)min(c, nc - 1) * Dout + o, w[WANT_DX ? u : 0][c]);
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (p0 + u < end) {
#pragma unroll
                    for (int c = 0; c < TC; ++c) {
                        if (WANT_DX) {
#pragma unroll
                            for (int q = 0; q < VEC; ++q) acc[c] = acc[c] + w[WANT_DX ? u : 0][c][q] * d[u][q];
                        }
                        if (WANT_DW && c < nc) {
                            float g[VEC];
#pragma unroll
                            for (int q = 0; q < VEC; ++q) g[q] = d[u][q] * xj[c];
                            Vec<VEC>::store(a.dwe + eo[u] + (int64_t)c * Dout + o, g);
                        }
                    }
                }
            }
        }
    }
    if (WANT_DX) {
        group_sum<TC>(acc, G);      // the group's lanes all hold the same row
        if (lig == 0) {
#pragma unroll
            for (int c = 0; c < TC; ++c)
                if (c < nc) a.dx[(int64_t)row * a.Din + c0 + c] = acc[c];
        }
    }
}

template <int VEC, bool WANT_DX, bool WANT_DW>
static void launch_nn_grad(const NnGradArgs &a, dim3 grid, hipStream_t stream) {
    constexpr int U = VEC == 4 ? 2 : 4;
    nn_grad_rows_kernel<VEC, U, WANT_DX, WANT_DW><<<grid, 64 * a.geom.waves, 0, stream>>>(a);
}

}  // namespace gnnmp

using namespace gnnmp;

extern "C" int gnnmp_nn_conv_grad_f32(const gnnmp_graph_t *plan_t, const gnnmp_nn_conv_grad_t *job, int64_t Din, int64_t Dout,
                                      gnnmp_stream_t stream) {
    if (!plan_t) return fail(GNNMP_EINVAL, "nn_conv_grad: null plan_t");
    if (!job) return fail(GNNMP_EINVAL, "nn_conv_grad: null job");
    if (!job->x) return fail(GNNMP_EINVAL, "nn_conv_grad: null x");
    if (!job->dm) return fail(GNNMP_EINVAL, "nn_conv_grad: null dm");
    if (!job->dx && !job->dwe) return fail(GNNMP_EINVAL, "nn_conv_grad: dx and dwe are both null: nothing to compute");
    if (job->dx && !job->we) return fail(GNNMP_EINVAL, "nn_conv_grad: dx without we");
    if (Din < 1 || Din > (1 << 16)) return fail(GNNMP_EINVAL, "nn_conv_grad: bad Din %lld", (long long)Din);
    if (Dout < 1 || Dout > (1 << 16)) return fail(GNNMP_EINVAL, "nn_conv_grad: bad Dout %lld", (long long)Dout);
    GNNMP_TRY(check_edge_plan("nn_conv_grad", plan_t, nullptr, true, "we has no row for them"));
    if (plan_t->n_dst == 0) return GNNMP_OK;
    if (!job->dx && plan_t->n_edges == 0) return GNNMP_OK;      // no row of dwe to write
    NnGradArgs a = {};
    a.rows = plan_rows_whole(plan_t);
    a.x = job->x;
    a.we = job->dx ? job->we : nullptr;
    a.dm = job->dm;
    a.dx = job->dx;
    a.dwe = job->dwe;
    a.Din = (int)Din;
    a.Dout = (int)Dout;
    // the lane width every vector access admits: o + Dout * c inside an edge's slab, for we (when read), dwe (when written) and Δ
    dim3 grid;
    const int vec = row_walk_geom("nn_conv_grad", a.rows, Dout, (int)((Din + NN_GRAD_TC - 1) / NN_GRAD_TC), {a.we, a.dwe, a.dm}, a.geom, grid);
    if (vec < 0) return vec;
    const bool want_dx = job->dx != nullptr, want_dw = job->dwe != nullptr;
    with_vec(vec, [&](auto V) {
        constexpr int VEC = decltype(V)::value;
        if (want_dx && want_dw)
            launch_nn_grad<VEC, true, true>(a, grid, (hipStream_t)stream);
        else if (want_dx)
            launch_nn_grad<VEC, true, false>(a, grid, (hipStream_t)stream);
        else
            launch_nn_grad<VEC, false, true>(a, grid, (hipStream_t)stream);
    });
    GNNMP_LAUNCH_CHECK("nn_grad_rows_kernel");
    return GNNMP_OK;
}
