// propagate.hip — the fused gather -> message -> per-destination reduce of GNNlib's propagate
// (GNNlib/src/msgpass.jl:71-79), i.e. apply_edges (:121-129: _gather(xj, s), message fn) followed by
// aggregate_neighbors (:145-149: _scatter(aggr, m, t, n)), without ever materialising the (D, E') message
// array.  Also the reference's SpMM fast path `xj * adjacency_matrix(g)` (:215-238): same kernel.
//
// HBM-bound (0.33-0.48 flop/B): the design goal is to keep every lane's 16-byte row loads in flight.
//   - one GROUP of G = 2^k lanes owns one destination row; lane l of the group owns VEC consecutive features
//     (G*VEC >= D; D=128 -> 32 lanes x float4, two rows per wave; D=100 -> 25 of 32 lanes active).
//   - the row's source ids (and the per-edge factors, when given in slot order) are loaded coalesced, G at a time,
//     one per lane, and broadcast inside the group with ds_bpermute (__shfl) — the CDNA cross-lane path, no LDS
//     allocation, no barrier.
//   - U row loads are issued back to back before the first add; the adds then run in ORIGINAL edge order,
//     one fp32 accumulator chain per feature => bit-identical to NNlib's CPU scatter loop, no atomics.
//   - rows longer than the plan's threshold are cut into balanced chunks (plan.hip); a chunk is processed by the SAME
//     kernel as a virtual row whose result goes to a partial buffer, and a small second kernel folds each long row's
//     partials in chunk order.  The dominant kernel therefore touches every edge exactly once and has no tail.
//   - block -> row-chunk mapping is XCD-aware (contiguous destination ranges per XCD / L2).
#include "csr_reduce.h"
#include "launch.h"

namespace gnnmp {

// one lane group per virtual row (rowwalk.h): a chunk of a long row leaves a raw partial, an ordinary row is finished here.
// FOLD: no second kernel for the split rows — the last chunk of a long row to arrive folds the row's partials itself, in the order of
// csr_combine_kernel (csr_reduce.h: chunk_arrive, fold_long_row).  One launch and one launch seam less per call: 5.6 us + the seam of a
// 107 us arxiv-shaped propagate.
template <int VEC, int OP, bool SCALED, int U, bool EMAT = false, bool EXPSUB = false, int GATED = 0, bool FOLD = false>
__global__ void __launch_bounds__(256) csr_rows_kernel(const ReduceArgs a) {
    VRow vr;   // (only the EXPSUB / GATED instances read a chunk's row)
    if (!decode_vrow<VROW_REMAP | VROW_ORDER | ((EXPSUB || GATED) ? 0 : VROW_NO_CHUNK_ROW)>(a.rows, a.geom, blockIdx.x, vr)) return;
    const int v = vr.v, lig = vr.lig, gbase = vr.gbase, G = vr.G;
    const int f0 = ((int)blockIdx.y * G + lig) * VEC;
    const bool active = f0 < a.D;
    float acc[VEC];
#pragma unroll
    for (int q = 0; q < VEC; ++q) acc[q] = op_identity<OP>();
    if (vr.is_chunk) {
        reduce_range<VEC, OP, SCALED, U, EMAT, EXPSUB, GATED>(a, vr.beg, vr.end, lig, gbase, G, f0, active, acc, vr.row);
        if (active) {
            if (FOLD) coh_store<VEC>(a.partial + (int64_t)v * a.D + f0, acc);      // read by another workgroup of this launch
            else Vec<VEC>::store(a.partial + (int64_t)v * a.D + f0, acc);
        }
        if (FOLD) {
            const int r = a.rows.chunk_lrow[v];
            const LongGeom lg = long_geom(a.rows.long_cptr, r, a.geom.log2g);
            const int NG = 256 >> a.geom.log2g;
            const int k = (v - lg.c0) / lg.per;
            const int s0 = lg.c0 + k * lg.per, s1 = min(lg.c1, s0 + lg.per);
            uint32_t *cnt = a.arrive + ((int64_t)r * gridDim.y + blockIdx.y) * (NG + 1);
            if (!chunk_arrive(cnt + k, s1 - s0, lig, gbase)) return;
            fold_rows<VEC, OP>(a.partial + (int64_t)s0 * a.D, a.D, s1 - s0, f0, active, acc, true);
            float *sp = a.spart + (int64_t)r * NG * a.D;
            if (active) coh_store<VEC>(sp + (int64_t)k * a.D + f0, acc);
            if (!chunk_arrive(cnt + NG, lg.ns, lig, gbase)) return;
            fold_rows<VEC, OP>(sp, a.D, lg.ns, f0, active, acc, false);
            const int lrow = a.rows.long_rows[r];
            finalize_store<VEC, OP>(a, lrow, a.rows.rowptr[lrow + 1] - a.rows.rowptr[lrow], f0, active, acc, a.compact_long ? r : -1);
        }
        return;
    }
    reduce_range<VEC, OP, SCALED, U, EMAT, EXPSUB, GATED>(a, vr.beg, vr.end, lig, gbase, G, f0, active, acc, vr.row);
    finalize_store<VEC, OP>(a, vr.row, vr.end - vr.beg, f0, active, acc);
}

// softmax_edge_neighbors, last step (GNNlib/src/utils.jl:96): alpha[k] = exp(e[k] - max_[t_k]) / den[t_k] for every edge of
// the (virtual) row, written back in ORIGINAL edge order.  idx = the plan's eid (rows of e / alpha).
template <int VEC, int U>
__global__ void __launch_bounds__(256) softmax_write_kernel(const ReduceArgs a) {
    VRow vr;
    if (!decode_vrow(a.rows, a.geom, blockIdx.x, vr)) return;
    const int row = vr.row, lig = vr.lig, gbase = vr.gbase, G = vr.G;
    const uint32_t beg = vr.beg, end = vr.end;
    const int f0 = ((int)blockIdx.y * G + lig) * VEC;
    const bool active = f0 < a.D;
    float mx[VEC], den[VEC];
#pragma unroll
    for (int q = 0; q < VEC; ++q) mx[q] = den[q] = 1.0f;
    if (active) {
        Vec<VEC>::load(a.rowsub + (int64_t)row * a.D + f0, mx);
        Vec<VEC>::load(a.rowden + (int64_t)row * a.D + f0, den);
    }
    if (a.den_add != 0.0f) {
#pragma unroll
        for (int q = 0; q < VEC; ++q) den[q] = den[q] + a.den_add;
    }
    float *outp = a.out;
    for (uint32_t base = beg; base < end; base += G) {   // slots are unsigned 32-bit (rowwalk.h)
        const uint32_t p = base + lig;
        const int c = p < end ? a.rows.col[p] : 0;
        const int n = (int)min((uint32_t)G, end - base);
        for (int j = 0; j < n; j += U) {
            float x[U][VEC];
            uint32_t cj[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                cj[u] = (uint32_t)__shfl(c, gbase + min(j + u, n - 1), 64);
                if (active) Vec<VEC>::load(a.x + (int64_t)cj[u] * a.D + f0, x[u]);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (active && (j + u < n)) {
#pragma unroll
                    for (int q = 0; q < VEC; ++q) x[u][q] = expf(x[u][q] - mx[q]) / den[q];
                    Vec<VEC>::store(outp + (int64_t)cj[u] * a.D + f0, x[u]);
                }
            }
        }
    }
}

// one BLOCK per long row: its 256 / G lane groups fold contiguous slices of the row's chunk partials (in chunk order, 8
// loads in flight), the slice results meet in LDS and group 0 folds them in slice order, then the usual epilogue.  (One
// lane group per row walked a 12 800-edge hub's 200 chunks alone: 14-40 us of a 250 us arxiv layer.)
template <int VEC, int OP>
__global__ void __launch_bounds__(256) csr_combine_kernel(const ReduceArgs a) {
    __shared__ float red[256 * VEC];
    const int G = 1 << a.geom.log2g;
    const int lig = threadIdx.x & (G - 1);
    const int grp = threadIdx.x >> a.geom.log2g;
    const int NG = 256 >> a.geom.log2g;
    const int r = blockIdx.x;
    const int f0 = ((int)blockIdx.y * G + lig) * VEC;
    const bool active = f0 < a.D;
    const int row = a.rows.long_rows[r];
    const int c0 = a.rows.long_cptr[r], c1 = a.rows.long_cptr[r + 1];
    const int per = (c1 - c0 + NG - 1) / NG;
    const int s0 = min(c1, c0 + grp * per), s1 = min(c1, s0 + per);
    float acc[VEC];
#pragma unroll
    for (int q = 0; q < VEC; ++q) acc[q] = op_identity<OP>();
    if (active) {
        constexpr int CB = 8;
        for (int c = s0; c < s1; c += CB) {
            float v[CB][VEC];
#pragma unroll
            for (int u = 0; u < CB; ++u) Vec<VEC>::load(a.partial + (int64_t)min(c + u, s1 - 1) * a.D + f0, v[u]);
#pragma unroll
            for (int u = 0; u < CB; ++u) {
                if (c + u < s1) {
#pragma unroll
                    for (int q = 0; q < VEC; ++q) acc[q] = op_apply<OP>(acc[q], v[u][q]);
                }
            }
        }
    }
#pragma unroll
    for (int q = 0; q < VEC; ++q) red[threadIdx.x * VEC + q] = acc[q];
    __syncthreads();
    if (grp != 0) return;
    for (int k = 1; k < NG; ++k) {
        if (c0 + k * per >= c1) break;               // empty slices hold the identity: nothing to fold
#pragma unroll
        for (int q = 0; q < VEC; ++q) acc[q] = op_apply<OP>(acc[q], red[((k << a.geom.log2g) + lig) * VEC + q]);
    }
    finalize_store<VEC, OP>(a, row, a.rows.rowptr[row + 1] - a.rows.rowptr[row], f0, active, acc, a.compact_long ? r : -1);
}

// nn_conv's propagate (GNNlib/src/layers/conv.jl:260-273): the message of edge k is W_k x_j with W_k = reshape(nn(e_k), out, in)
// — an (out, in) matrix PER EDGE, read once, by original edge position (`we`, Julia column-major: element (o, c) at o + out * c).
// One group of G >= out lanes per destination (virtual) row, lane o owns output feature o: for every in-channel the out
// weights of the edge are one contiguous, coalesced load and x_j[c] is a broadcast.  Edges in original order, products
// rounded then added (the reference runs a batched gemm: tolerance, not bits).  Chunks of long rows leave raw partials for
// csr_combine_kernel like every other row kernel.
template <int OP>
__global__ void __launch_bounds__(256) nn_rows_kernel(const ReduceArgs a, const float *__restrict__ we, int Din) {
    VRow vr;
    if (!decode_vrow<VROW_NO_CHUNK_ROW>(a.rows, a.geom, blockIdx.x, vr)) return;
    const int v = vr.v, row = vr.row;
    const bool is_chunk = vr.is_chunk;
    const uint32_t beg = vr.beg, end = vr.end;
    const int o = (int)blockIdx.y * vr.G + vr.lig;
    const bool active = o < a.D;
    float acc = op_identity<OP>();
    const int oc = active ? o : 0;
    // EB edges at a time: their EB x 2 in-channel loads are independent (a row walks its edges alone — with one edge in flight
    // the kernel ran at a third of the HBM rate); messages are still formed per edge and folded in edge order.  Slots past
    // the end re-read the last edge and are not folded.
    constexpr int EB = 4;
    for (uint32_t p0 = beg; p0 < end; p0 += EB) {
        const float *wk[EB], *xr[EB];
        bool ok[EB];
#pragma unroll
        for (int u = 0; u < EB; ++u) {
            const uint32_t p = min(p0 + u, end - 1);
            const int cj = a.rows.col[p];
            const uint32_t ej = (uint32_t)a.rows.eid[p];
            ok[u] = p0 + u < end && ej < a.rows.n_edges;          // a self loop the plan added: no edge features, no message
            wk[u] = we + (int64_t)(a.rows.n_edges ? min(ej, a.rows.n_edges - 1) : 0u) * a.D * Din + oc;
            xr[u] = a.x + (int64_t)cj * Din;
        }
        float m[EB];
#pragma unroll
        for (int u = 0; u < EB; ++u) m[u] = 0.0f;
        int c = 0;
        for (; c + 2 <= Din; c += 2) {
            float w0[EB], w1[EB], x0[EB], x1[EB];
#pragma unroll
            for (int u = 0; u < EB; ++u) {
                w0[u] = wk[u][(int64_t)c * a.D];
                w1[u] = wk[u][(int64_t)(c + 1) * a.D];
                x0[u] = xr[u][c];
                x1[u] = xr[u][c + 1];
            }
#pragma unroll
            for (int u = 0; u < EB; ++u) {
                m[u] = m[u] + w0[u] * x0[u];
                m[u] = m[u] + w1[u] * x1[u];
            }
        }
        if (c < Din) {
#pragma unroll
            for (int u = 0; u < EB; ++u) m[u] = m[u] + wk[u][(int64_t)c * a.D] * xr[u][c];
        }
#pragma unroll
        for (int u = 0; u < EB; ++u)
            if (ok[u]) acc = op_apply<OP>(acc, m[u]);
    }
    if (is_chunk) {
        if (active) a.partial[(int64_t)v * a.D + o] = acc;
        return;
    }
    float av[1] = {acc};
    finalize_store<1, OP>(a, row, end - beg, o, active, av);
}

template <int VEC, int OP, bool SCALED, int U, bool EMAT = false, bool EXPSUB = false, int GATED = 0>
static int launch_reduce(const ReduceArgs &a0, hipStream_t stream) {
    ReduceArgs a = a0;
    const int waves = block_waves(4);
    a.geom.waves = waves;
    const int tiles = feature_tiles(a.D, VEC, a.geom.log2g);
    const dim3 grid = row_grid(a.rows, a.geom, tiles, use_xcd_remap(a.n_src, a.D, row_blocks(a.rows, a.geom)));
    if (grid.x > 0) {
        // the plain propagate / scatter instances fold their split rows themselves (a.arrive set by run_reduce when it may)
        constexpr bool CAN_FOLD = !EMAT && !EXPSUB && GATED == 0 && U == 8;
        if (CAN_FOLD && a.arrive && a.rows.n_long > 0) {
            csr_rows_kernel<VEC, OP, SCALED, U, EMAT, EXPSUB, GATED, CAN_FOLD><<<grid, 64 * waves, 0, stream>>>(a);
            GNNMP_LAUNCH_CHECK("csr_rows_kernel<FOLD>");
            return GNNMP_OK;
        }
        csr_rows_kernel<VEC, OP, SCALED, U, EMAT, EXPSUB, GATED><<<grid, 64 * waves, 0, stream>>>(a);
        GNNMP_LAUNCH_CHECK("csr_rows_kernel");
    }
    if (a.rows.n_long > 0) {
        dim3 cg((unsigned)a.rows.n_long, (unsigned)tiles);
        csr_combine_kernel<VEC, OP><<<cg, 256, 0, stream>>>(a);
        GNNMP_LAUNCH_CHECK("csr_combine_kernel");
    }
    return GNNMP_OK;
}

template <int VEC, int OP, bool SCALED>
static int dispatch_u(const ReduceArgs &a, hipStream_t s) {
    switch (knob(KNOB_UNROLL)) {
        case 2: return launch_reduce<VEC, OP, SCALED, 2>(a, s);
        case 4: return launch_reduce<VEC, OP, SCALED, 4>(a, s);
        default: return launch_reduce<VEC, OP, SCALED, 8>(a, s);
    }
}
template <int VEC, int OP>
static int dispatch_scaled(const ReduceArgs &a, bool scaled, hipStream_t s) {
    return scaled ? dispatch_u<VEC, OP, true>(a, s) : dispatch_u<VEC, OP, false>(a, s);
}
template <int VEC>
static int dispatch_op(const ReduceArgs &a, int op, bool scaled, hipStream_t s) {
    if (a.rowsub) return launch_reduce<VEC, OP_SUM, false, 8, false, true>(a, s);   // softmax denominator
    if (a.gate_i && a.gated == 2) {   // cg_conv aggregates with + (conv.jl:313)
        return a.emat ? launch_reduce<VEC, OP_SUM, false, 2, true, false, 2>(a, s)
                      : launch_reduce<VEC, OP_SUM, false, 4, false, false, 2>(a, s);
    }
    if (a.gate_i) {   // two rows per edge in flight: half the batch
        switch (op) {
            case OP_SUM: return launch_reduce<VEC, OP_SUM, false, 4, false, false, 1>(a, s);
            case OP_MAX: return launch_reduce<VEC, OP_MAX, false, 4, false, false, 1>(a, s);
            default: return launch_reduce<VEC, OP_MIN, false, 4, false, false, 1>(a, s);
        }
    }
    if (a.emat) {   // two rows per edge in flight: half the batch
        switch (op) {
            case OP_SUM: return launch_reduce<VEC, OP_SUM, false, 4, true>(a, s);
            case OP_MAX: return launch_reduce<VEC, OP_MAX, false, 4, true>(a, s);
            default: return launch_reduce<VEC, OP_MIN, false, 4, true>(a, s);
        }
    }
    switch (op) {
        case OP_SUM: return dispatch_scaled<VEC, OP_SUM>(a, scaled, s);
        case OP_MAX: return dispatch_scaled<VEC, OP_MAX>(a, scaled, s);
        default: return dispatch_scaled<VEC, OP_MIN>(a, scaled, s);
    }
}

int run_reduce(gnnmp_graph_t *p, const ReduceCall &c, hipStream_t stream) {
    const int64_t D = c.D;
    const int long_only = c.long_only;
    if (p->n_dst == 0 || D == 0) return GNNMP_OK;
    if (long_only && p->n_long == 0) return GNNMP_OK;
    if (p->n_chunks > 0 && !long_only) {
        if (int rc = ensure_workspace(p, (size_t)p->n_chunks * (size_t)D)) return rc;
    }
    ReduceArgs a;
    a.compact_long = long_only;
    a.rows = plan_rows(p);
    a.rows.col = c.idx;
    if (long_only) a.rows.n_rows = 0;
    a.x = c.x;
    a.w = c.w;
    a.emat = c.emat;
    a.rowsub = c.rowsub;
    a.rowden = nullptr;
    a.den_add = 0.0f;
    a.gate_i = c.gate_i;
    a.gated = c.gate_i ? c.gated : 0;
    a.act = c.act;
    a.ss = c.ss;
    a.w_slot = c.w_slot;
    a.ss_slot = c.ss_slot;
    a.sd = c.sd;
    a.out = c.out;
    a.bias = c.bias;
    a.bias_relu = c.bias_relu;
    a.addend = c.addend;
    a.mask_y = c.mask_y;
    a.partial = p->ws;
    a.D = (int)D;
    a.n_src = (int)p->n_src;
    a.mean = (c.aggr == GNNMP_MEAN);
    a.geom = RowGeom{0, 4, 0, 0};
    a.arrive = nullptr;
    const int vec = narrow_vec(pick_vec(D, c.x, c.out), c.addend, c.mask_y, c.emat, c.gate_i);
    a.geom.log2g = pick_log2g((D + vec - 1) / vec);
    // >= 2 rows per wave: pair rows of equal length — but only when an output row is whole 128-byte lines: out of index order,
    // rows of 400 bytes (D = 100) leave every line half written by one wave and finished by another, measured 4.75 -> 5.11 ms
    if (!long_only && use_row_order(p->n_src, D) && a.geom.log2g <= 5 && c.idx == p->col && (D & 31) == 0 &&
        (reinterpret_cast<uintptr_t>(c.out) & 127) == 0) {
        if (int rc = ensure_row_order(p, stream)) return rc;
        a.rows.row_order = p->row_order;
    }
    const int op = (c.aggr == GNNMP_MAX) ? OP_MAX : (c.aggr == GNNMP_MIN ? OP_MIN : OP_SUM);
    const bool scaled = c.w || c.ss || c.w_slot || c.ss_slot;
    a.spart = nullptr;
    if (p->n_long > 0 && use_fold()) {      // split rows folded inside the row kernel: arrival counters per (long row, feature tile, slice)
        const int NG = 256 >> a.geom.log2g;
        const size_t tiles = (size_t)feature_tiles(D, vec, a.geom.log2g);
        if (int rc = ensure_arrive(p, (size_t)p->n_long * tiles * (size_t)(NG + 1), (size_t)p->n_long * (size_t)NG * (size_t)D, stream)) return rc;
        a.arrive = p->arrive;
        a.spart = p->spart;
    }
    return with_vec(vec, [&](auto V) { return dispatch_op<decltype(V)::value>(a, op, scaled, stream); });
}

// softmax over the rows of a plan in the reference's three steps (utils.jl:84-97 / :49-72): max_ = scatter(max, e, t),
// den = scatter(+, exp.(e .- max_[t]), t) (edge order), alpha = num ./ den.  Every step is the balanced row-group walk
// (chunked long rows), so a 17 000-edge hub costs what 17 000 edges cost, not a serial tail.
int run_softmax(gnnmp_graph_t *p, const float *e, float *alpha, int64_t D, float den_add, hipStream_t stream) {
    if (p->n_dst == 0 || p->n_total == 0 || D == 0) return GNNMP_OK;
    const size_t nd = (size_t)p->n_dst * (size_t)D, pc = (size_t)p->n_chunks * (size_t)D;
    if (int rc = ensure_workspace(p, pc + 2 * nd)) return rc;
    float *mx = p->ws + pc, *den = mx + nd;
    // narrow rows: one pass over the rows the plan does not split, a wave per chunk on those it does (softmax_rows.hip)
    const int rc1 = softmax_rows_try(p, e, alpha, D, den_add, p->ws, mx, den, stream);
    if (rc1 != 1) return rc1;
    ReduceCall c;
    c.idx = p->eid;
    c.x = e;
    c.D = D;
    c.aggr = GNNMP_MAX;
    c.out = mx;
    if (int rc = run_reduce(p, c, stream)) return rc;
    c.aggr = GNNMP_SUM;
    c.rowsub = mx;
    c.out = den;
    if (int rc = run_reduce(p, c, stream)) return rc;
    ReduceArgs a = {};
    a.rows = plan_rows(p);
    a.rows.col = p->eid;      // rows of e / alpha: by original edge position
    a.x = e;
    a.out = alpha;
    a.rowsub = mx;
    a.rowden = den;
    a.den_add = den_add;
    a.D = (int)D;
    const int vec = pick_vec(D, e, alpha);
    a.geom = RowGeom{pick_log2g((D + vec - 1) / vec), 4, 0, 0};
    const dim3 grid = row_grid(a.rows, a.geom, feature_tiles(D, vec, a.geom.log2g));
    with_vec(vec, [&](auto V) { softmax_write_kernel<decltype(V)::value, 8><<<grid, 64 * a.geom.waves, 0, stream>>>(a); });
    GNNMP_LAUNCH_CHECK("softmax_write_kernel");
    return GNNMP_OK;
}

int run_combine(gnnmp_graph_t *p, float *out, int64_t D, int aggr, hipStream_t stream) {
    if (p->n_long == 0) return GNNMP_OK;
    ReduceArgs a = {};
    a.rows = plan_rows(p);
    a.out = out;
    a.partial = p->ws;
    a.D = (int)D;
    const int vec = pick_vec(D, p->ws, out);
    a.geom.log2g = pick_log2g((D + vec - 1) / vec);
    dim3 grid((unsigned)a.rows.n_long, (unsigned)feature_tiles(D, vec, a.geom.log2g));
    with_vec(vec, [&](auto V) {
        constexpr int VEC = decltype(V)::value;
        if (aggr == GNNMP_MAX)
            csr_combine_kernel<VEC, OP_MAX><<<grid, 256, 0, stream>>>(a);
        else
            csr_combine_kernel<VEC, OP_SUM><<<grid, 256, 0, stream>>>(a);
    });
    GNNMP_LAUNCH_CHECK("csr_combine_kernel");
    return GNNMP_OK;
}

// ---- degree / norm ------------------------------------------------------------------------------
__global__ void degree_count_kernel(const uint32_t *rowptr, int64_t n, float *deg) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) deg[i] = 0.0f + (float)(rowptr[i + 1] - rowptr[i]);
}
// weighted in-degree: one thread per destination, weights added in original edge order
// (zeros(T,N) .+ scatter(+, w, t) — GNNGraphs/src/query.jl:359-369)
__global__ void degree_weighted_kernel(const uint32_t *rowptr, const int32_t *eid, const float *w,
                                       int64_t n, uint32_t n_edges, float *deg, int long_thresh) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t beg = rowptr[i], end = rowptr[i + 1];
    if (end - beg > long_thresh) return;   // split rows: degree_long_kernel (a 17 000-edge hub made this thread a 5.6 ms tail)
    float acc = 0.0f;
    int64_t p = beg;
    for (; p + 8 <= end; p += 8) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const uint32_t e = (uint32_t)eid[p + u];
            v[u] = e < n_edges ? w[e] : 1.0f;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) acc = acc + v[u];
    }
    for (; p < end; ++p) {
        const uint32_t e = (uint32_t)eid[p];
        acc = acc + (e < n_edges ? w[e] : 1.0f);
    }
    deg[i] = 0.0f + acc;
}
// weighted in-degree of the split rows: one block per long row, threads stride over its slots, fixed-shape LDS tree
__global__ void __launch_bounds__(256) degree_long_kernel(const uint32_t *rowptr, const int32_t *eid, const float *w,
                                                          const int32_t *long_rows, uint32_t n_edges, float *deg) {
    __shared__ float red[256];
    const int row = long_rows[blockIdx.x];
    const int64_t beg = rowptr[row], end = rowptr[row + 1];
    float acc = 0.0f;
    for (int64_t p = beg + (int)threadIdx.x; p < end; p += 256) {
        const uint32_t e = (uint32_t)eid[p];
        acc = acc + (e < n_edges ? w[e] : 1.0f);
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] = red[threadIdx.x] + red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) deg[row] = 0.0f + red[0];
}
__global__ void inv_sqrt_kernel(const float *deg, float *out, int64_t n) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    // plain sqrtf and '/': hipcc's default -fhip-fp32-correctly-rounded-divide-sqrt makes both IEEE-rounded
    // (HIP's __fsqrt_rn maps to the native, 1-ulp sqrt: measured 13 % mismatches vs the CPU).
    if (i < n) out[i] = 1.0f / sqrtf(deg[i]);
}

}  // namespace gnnmp

using namespace gnnmp;

// What the propagate / scatter exports check first, in this order: the plan, aggr, D in [0, max_D], and the two arrays every one
// of them needs — `in` where the plan has slots, and `out` (`io` names them in the message).  What only one export checks stays there.
static int check_rows_call(const char *who, const gnnmp_graph_t *plan, int aggr, int64_t D, int64_t max_D, const float *in,
                           const float *out, const char *io = "xj/out") {
    if (!plan) return fail(GNNMP_EINVAL, "%s: null plan", who);
    if (aggr < GNNMP_SUM || aggr > GNNMP_MIN) return fail(GNNMP_EINVAL, "%s: bad aggr %d", who, aggr);
    if (D < 0 || D > max_D) return fail(GNNMP_EINVAL, "%s: bad D %lld", who, (long long)D);
    if (plan->n_dst > 0 && D > 0 && (!out || (!in && plan->n_total > 0))) return fail(GNNMP_EINVAL, "%s: null %s", who, io);
    return GNNMP_OK;
}
// a propagate over the plan's sources: what every export below starts its ReduceCall from
static ReduceCall propagate_call(const gnnmp_graph_t *plan, int aggr, const float *xj, float *out, int64_t D) {
    ReduceCall c;
    c.idx = plan->col;
    c.aggr = aggr;
    c.x = xj;
    c.out = out;
    c.D = D;
    return c;
}

extern "C" {

int gnnmp_propagate_f32(gnnmp_graph_t *plan, int msg, int aggr, const float *xj, const float *w,
                        const float *scale_src, const float *scale_dst, float *out, int64_t D,
                        gnnmp_stream_t stream) {
    if (int rc = check_rows_call("propagate", plan, aggr, D, 1 << 20, xj, out)) return rc;
    if (msg != GNNMP_COPY_XJ && msg != GNNMP_W_MUL_XJ) return fail(GNNMP_EINVAL, "propagate: bad msg %d", msg);
    if (msg == GNNMP_W_MUL_XJ && !w && plan->n_edges > 0)
        return fail(GNNMP_EINVAL, "propagate: W_MUL_XJ needs w");
    ReduceCall c = propagate_call(plan, aggr, xj, out, D);
    if (msg == GNNMP_W_MUL_XJ) c.w = w;
    c.ss = scale_src;
    c.sd = scale_dst;
    return run_reduce(plan, c, (hipStream_t)stream);
}

int gnnmp_propagate_emul_f32(gnnmp_graph_t *plan, int aggr, const float *xj, const float *e, float *out, int64_t D,
                             gnnmp_stream_t stream) {
    if (int rc = check_rows_call("propagate_emul", plan, aggr, D, 1 << 20, xj, out, "xj/e/out")) return rc;
    if (plan->n_dst > 0 && D > 0 && !e && plan->n_edges > 0) return fail(GNNMP_EINVAL, "propagate_emul: null xj/e/out");
    ReduceCall c = propagate_call(plan, aggr, xj, out, D);
    c.emat = e;
    return run_reduce(plan, c, (hipStream_t)stream);
}

int gnnmp_propagate_gated_f32(gnnmp_graph_t *plan, int aggr, const float *gate_i, const float *bv_j, float *out, int64_t D,
                              gnnmp_stream_t stream) {
    if (int rc = check_rows_call("propagate_gated", plan, aggr, D, 1 << 19, bv_j, out, "pointer")) return rc;
    if (plan->n_dst > 0 && D > 0 && !gate_i) return fail(GNNMP_EINVAL, "propagate_gated: null pointer");
    ReduceCall c = propagate_call(plan, aggr, bv_j, out, D);
    c.gate_i = gate_i;
    return run_reduce(plan, c, (hipStream_t)stream);
}

int gnnmp_propagate_cg_f32(gnnmp_graph_t *plan, const float *fs_i, const float *fs_j, const float *fs_e, int act, float *out,
                           int64_t D, gnnmp_stream_t stream) {
    if (int rc = check_rows_call("propagate_cg", plan, GNNMP_SUM, D, 1 << 19, fs_j, out, "pointer")) return rc;
    if (act < GNNMP_ACT_IDENTITY || act > GNNMP_ACT_TANH) return fail(GNNMP_EINVAL, "propagate_cg: bad act %d", act);
    if (plan->n_dst > 0 && D > 0 && !fs_i) return fail(GNNMP_EINVAL, "propagate_cg: null pointer");
    ReduceCall c = propagate_call(plan, GNNMP_SUM, fs_j, out, D);
    c.emat = fs_e;
    c.gate_i = fs_i;
    c.gated = 2;
    c.act = act;
    return run_reduce(plan, c, (hipStream_t)stream);
}

int gnnmp_propagate_nn_f32(gnnmp_graph_t *p, int aggr, const float *xj, const float *we, float *out, int64_t Din, int64_t Dout,
                           gnnmp_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!p) return fail(GNNMP_EINVAL, "propagate_nn: null plan");
    if (aggr < GNNMP_SUM || aggr > GNNMP_MIN) return fail(GNNMP_EINVAL, "propagate_nn: bad aggr %d", aggr);
    if (Din <= 0 || Dout <= 0 || Din > (1 << 16) || Dout > (1 << 16)) return fail(GNNMP_EINVAL, "propagate_nn: bad size");
    if (p->n_dst == 0) return GNNMP_OK;
    if (!out || ((!xj || !we) && p->n_total > 0)) return fail(GNNMP_EINVAL, "propagate_nn: null pointer");
    if (p->n_chunks > 0) {
        if (int rc = ensure_workspace(p, (size_t)p->n_chunks * (size_t)Dout)) return rc;
    }
    ReduceArgs a = {};
    a.rows = plan_rows(p);
    a.x = xj;
    a.out = out;
    a.partial = p->ws;
    a.D = (int)Dout;
    a.n_src = (int)p->n_src;
    a.mean = (aggr == GNNMP_MEAN);
    a.geom = RowGeom{pick_log2g(Dout), 4, 0, 0};
    const int tiles = feature_tiles(Dout, 1, a.geom.log2g);
    const dim3 grid = row_grid(a.rows, a.geom, tiles);
    const int op = (aggr == GNNMP_MAX) ? OP_MAX : (aggr == GNNMP_MIN ? OP_MIN : OP_SUM);
    with_op(op, [&](auto O) { nn_rows_kernel<decltype(O)::value><<<grid, 64 * a.geom.waves, 0, stream>>>(a, we, (int)Din); });
    GNNMP_LAUNCH_CHECK("nn_rows_kernel");
    if (a.rows.n_long > 0) {
        dim3 cg((unsigned)a.rows.n_long, (unsigned)tiles);
        with_op(op, [&](auto O) { csr_combine_kernel<1, decltype(O)::value><<<cg, 256, 0, stream>>>(a); });
        GNNMP_LAUNCH_CHECK("csr_combine_kernel");
    }
    return GNNMP_OK;
}

int gnnmp_propagate_slots_f32(gnnmp_graph_t *plan, int aggr, const float *xj, const float *w_slot,
                              const float *ss_slot, const float *scale_dst, float *out, int64_t D,
                              gnnmp_stream_t stream) {
    if (int rc = check_rows_call("propagate_slots", plan, aggr, D, 1 << 20, xj, out)) return rc;
    ReduceCall c = propagate_call(plan, aggr, xj, out, D);
    c.w_slot = w_slot;
    c.ss_slot = ss_slot;
    c.sd = scale_dst;
    return run_reduce(plan, c, (hipStream_t)stream);
}

int gnnmp_propagate_slots_act_f32(gnnmp_graph_t *plan, int aggr, const float *xj, const float *w_slot, const float *ss_slot,
                                  const float *scale_dst, const float *bias, int act, float *out, int64_t D,
                                  gnnmp_stream_t stream) {
    if (int rc = check_rows_call("propagate_slots_act", plan, aggr, D, 1 << 20, xj, out)) return rc;
    if (act != GNNMP_ACT_IDENTITY && act != GNNMP_ACT_RELU) return fail(GNNMP_EINVAL, "propagate_slots_act: bad act %d", act);
    ReduceCall c = propagate_call(plan, aggr, xj, out, D);
    c.w_slot = w_slot;
    c.ss_slot = ss_slot;
    c.sd = scale_dst;
    c.bias = bias;
    c.bias_relu = act == GNNMP_ACT_RELU ? 1 : 0;
    return run_reduce(plan, c, (hipStream_t)stream);
}

/* out = act'( addend + aggregate ): the tail of graph_conv's / sage_conv's pullback w.r.t. x in the row kernel's epilogue (gnnmp.h) */
int gnnmp_propagate_add_mask_f32(gnnmp_graph_t *plan, int aggr, const float *xj, const float *scale_dst, const float *addend,
                                 const float *mask_y, float *out, int64_t D, gnnmp_stream_t stream) {
    const bool sum_or_mean = aggr == GNNMP_SUM || aggr == GNNMP_MEAN;   // (its own message for aggr, below)
    if (int rc = check_rows_call("propagate_add_mask", plan, sum_or_mean ? aggr : GNNMP_SUM, D, 1 << 20, xj, out)) return rc;
    if (!sum_or_mean) return fail(GNNMP_EINVAL, "propagate_add_mask: aggr must be + or mean (got %d)", aggr);
    ReduceCall c = propagate_call(plan, aggr, xj, out, D);
    c.sd = scale_dst;
    c.addend = addend;
    c.mask_y = mask_y;
    return run_reduce(plan, c, (hipStream_t)stream);
}

int gnnmp_scatter_f32(gnnmp_graph_t *plan, int aggr, const float *m, float *out, int64_t D,
                      gnnmp_stream_t stream) {
    if (int rc = check_rows_call("scatter", plan, aggr, D, 1 << 20, m, out, "m/out")) return rc;
    ReduceCall c = propagate_call(plan, aggr, m, out, D);
    c.idx = plan->eid;      // rows of m: by original edge position
    return run_reduce(plan, c, (hipStream_t)stream);
}

int gnnmp_degree_f32(gnnmp_graph_t *plan, const float *w, float *deg, gnnmp_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!plan) return fail(GNNMP_EINVAL, "degree: null plan");
    if (plan->n_dst == 0) return GNNMP_OK;
    if (!deg) return fail(GNNMP_EINVAL, "degree: null output");
    const unsigned nb = (unsigned)((plan->n_dst + 255) / 256);
    if (w) {
        degree_weighted_kernel<<<nb, 256, 0, stream>>>(plan->rowptr, plan->eid, w, plan->n_dst,
                                                        (uint32_t)plan->n_edges, deg, plan->long_thresh);
        if (plan->n_long > 0)
            degree_long_kernel<<<(unsigned)plan->n_long, 256, 0, stream>>>(plan->rowptr, plan->eid, w, plan->long_rows,
                                                                            (uint32_t)plan->n_edges, deg);
    } else
        degree_count_kernel<<<nb, 256, 0, stream>>>(plan->rowptr, plan->n_dst, deg);
    GNNMP_LAUNCH_CHECK("degree kernel");
    return GNNMP_OK;
}

int gnnmp_inv_sqrt_f32(const float *deg, float *out, int64_t n, gnnmp_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (n < 0) return fail(GNNMP_EINVAL, "inv_sqrt: negative n");
    if (n == 0) return GNNMP_OK;
    if (!deg || !out) return fail(GNNMP_EINVAL, "inv_sqrt: null pointer");
    inv_sqrt_kernel<<<(unsigned)((n + 255) / 256), 256, 0, stream>>>(deg, out, n);
    GNNMP_LAUNCH_CHECK("inv_sqrt_kernel");
    return GNNMP_OK;
}

}  // extern "C"
