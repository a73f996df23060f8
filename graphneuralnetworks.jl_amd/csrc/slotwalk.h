// slotwalk.h — the pieces every kernel shares that walks the rows of a plan with one lane group a row: the training kernels of
// edge_conv.hip, cg_grad.hip, nn_grad.hip, egnn.hip, gmm.hip and megnet.hip, maxmin_grad.h, linkpred.hip's row_accumulate and the hop of
// poly_conv.hip.
//
// What a whole-row walk is.  No atomics, no plan-owned scratch, every output element written exactly once (rows without in-edges and
// rows without out-edges included).  The kernels walk every row WHOLE, in slot order — original edge order — whatever its length: their
// PlanRows is plan_rows_whole's (no chunk virtual rows) and decode_vrow is told not to skip the rows longer than long_thresh
// (VROW_WHOLE).  Every sum therefore has the bits of the sequential fold and two calls give equal bits; the price is that A HUB ROW IS
// WALKED BY ONE LANE GROUP: correct, slow.
//
// Chunked hub rows (the split route).  A kernel whose aggregate is a plain sum can walk plan_rows(plan) instead — decode_row_lane<VEC, 0>
// (or VROW_NO_CHUNK_ROW): the chunk virtual rows [0, n_chunks) come first, a row longer than long_thresh is skipped — and needs three more
// pieces, all here: a chunk's lane group stores its UNSCALED partial with store_partial into a CALLER-GIVEN workspace [n_chunks][width]
// (never the plan's: the plan stays read-only and two streams may share it); a second launch gives every split row a lane group
// (decode_long_lane), adds the row's partials IN CHUNK ORDER with fold_partials — a fixed order, so two calls give equal bits — and runs
// the kernel's own epilogue.  Still no atomics, and every workspace element a fold reads was written by the launch before it: nothing
// needs clearing, a capture needs no eager call first.  A row up to long_thresh takes the very same instructions as in a whole-row walk
// and keeps its bits; a split row's sum is grouped by chunk and owes its kernel's error bar, not the sequential fold's bits.
// TODAY ONLY poly_hop_kernel (poly_conv.hip) HAS THE SPLIT ROUTE.  edge_conv.hip, cg_grad.hip, nn_grad.hip, egnn.hip, gmm.hip, megnet.hip,
// maxmin_grad.h and linkpred.hip still walk every row whole; the pieces below are what each of them takes when its turn comes.
//
// The shape of a walk (the two loops stay in the kernel: it declares its in-flight buffers between them, at kernel scope — walks that
// own the buffers, or take the body as a callback, cost registers, waves or scratch: LABNOTES.md, 2026-10-20):
//     RowLane w;
//     if (!decode_row_lane<VEC>(a.rows, a.geom, width, w)) return;
//     for (uint32_t base = w.beg; base < w.end; base += w.G) {            // a batch: one slot a lane
//         const Slots s = load_slots<COL, EID>(a.rows.col, a.rows.eid, base, w.end, w.lig, w.G);
//         for (int j = 0; j < s.n; j += U) {                              // U slots in flight
//             bcast_slots<U, COL, EID>(s, w.gbase, j, cjs, ejs);          // slots past the batch's end repeat its last one: every
//             ... load_or_zero<VEC>(w.active, x + (int64_t)cjs[u] * ld + w.f0, v[u]) ...   // load below has a valid address,
//             ... if (j + u < s.n) use v[u] ...                           // unconditional within the lane's activity
//         }
//     }
// Slots are unsigned 32-bit (rowwalk.h).  An eid read here is < n_edges: the exports refuse a plan with self loops of its own
// (check_edge_plan, launch.h).
#pragma once
#include "rowwalk.h"

namespace gnnmp {

// A decoded virtual row and the calling lane's place in its feature tile: VEC features from f0 on; the lanes of the last tile that lie
// past the width are not active — they load nothing and store nothing, and still take part in every shuffle.
struct RowLane : VRow {
    int f0;
    bool active;
};
template <int VEC, int FLAGS = VROW_WHOLE>
__device__ __forceinline__ bool decode_row_lane(const PlanRows &r, const RowGeom &g, int width, RowLane &w) {
    if (!decode_vrow<FLAGS>(r, g, blockIdx.x, w)) return false;
    w.f0 = ((int)blockIdx.y * w.G + w.lig) * VEC;
    w.active = w.f0 < width;
    return true;
}

// One batch of a row: lane lig holds slot base + lig (c = col, ev = eid; zeros past the row's end), n = the slots of the batch.
struct Slots {
    int c;
    uint32_t ev;
    int n;
};
template <bool COL, bool EID>
__device__ __forceinline__ Slots load_slots(const int32_t *col, const int32_t *eid, uint32_t base, uint32_t end, int lig, int G) {
    const uint32_t p = base + lig;
    Slots s = {0, 0u, (int)min((uint32_t)G, end - base)};
    if (p < end) {
        if (COL) s.c = col[p];
        if (EID) s.ev = (uint32_t)eid[p];
    }
    return s;
}
// out[u] = the word lane j + u of the group holds, clamped to the batch's last slot — for anything a kernel keeps one per slot
template <int U, class T>
__device__ __forceinline__ void bcast_word(T v, int n, int gbase, int j, T (&out)[U]) {
#pragma unroll
    for (int u = 0; u < U; ++u) out[u] = __shfl(v, gbase + min(j + u, n - 1), 64);
}
template <int U, bool COL, bool EID>
__device__ __forceinline__ void bcast_slots(const Slots &s, int gbase, int j, int (&cjs)[U], uint32_t (&ejs)[U]) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int jj = min(j + u, s.n - 1);
        cjs[u] = COL ? __shfl(s.c, gbase + jj, 64) : 0;
        ejs[u] = EID ? (uint32_t)__shfl((int)s.ev, gbase + jj, 64) : 0u;
    }
}

template <int VEC>
__device__ __forceinline__ void load_or_zero(bool active, const float *p, float v[VEC]) {
    if (active) {
        Vec<VEC>::load(p, v);
    } else {
#pragma unroll
        for (int q = 0; q < VEC; ++q) v[q] = 0.0f;
    }
}

// ---- chunked hub rows: the partial of a chunk and the fold of a split row ----------------------------------------------------------------
// partial[v][width]: row v of the workspace is chunk virtual row v's; a lane's VEC floats lie at f0 like its row's in out, so that the
// feature tiles (blockIdx.y) index the workspace as they index out.  width % VEC == 0 whenever VEC > 1 (pick_vec): a partial row is
// aligned when the workspace is.
template <int VEC>
__device__ __forceinline__ void store_partial(float *partial, int width, const RowLane &w, const float acc[VEC]) {
    Vec<VEC>::store(partial + (int64_t)w.v * width + w.f0, acc);
}

// The calling lane's place in the FOLD launch: lane group l of the grid takes split row long_rows[l] and its chunks [c0, c1), the lanes
// run over the features as in decode_row_lane.  false = nothing to do (past the last split row).  Grid: long_grid.
struct LongLane {
    int row;          // the destination
    int c0, c1;       // its chunk virtual rows, in slot order
    int f0;
    bool active;
};
template <int VEC>
__device__ __forceinline__ bool decode_long_lane(const PlanRows &r, const RowGeom &g, int width, LongLane &w) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lig = lane & ((1 << g.log2g) - 1);
    const int64_t l = ((int64_t)blockIdx.x * g.waves + wave) * (64 >> g.log2g) + (lane >> g.log2g);
    if (l >= r.n_long) return false;
    w.row = r.long_rows[l];
    w.c0 = r.long_cptr[l];
    w.c1 = r.long_cptr[l + 1];
    w.f0 = ((int)blockIdx.y * (1 << g.log2g) + lig) * VEC;
    w.active = w.f0 < width;
    return true;
}
// acc = ((0 + p[c0]) + p[c0 + 1]) + ... + p[c1 - 1], U partial rows in flight; a load past the last chunk repeats it (a valid address,
// unconditional) and is not added.  Only for an active lane.
template <int VEC, int U>
__device__ __forceinline__ void fold_partials(const float *partial, int width, const LongLane &w, float acc[VEC]) {
#pragma unroll
    for (int q = 0; q < VEC; ++q) acc[q] = 0.0f;
    for (int c = w.c0; c < w.c1; c += U) {
        float v[U][VEC];
#pragma unroll
        for (int u = 0; u < U; ++u) Vec<VEC>::load(partial + (int64_t)min(c + u, w.c1 - 1) * width + w.f0, v[u]);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (c + u < w.c1) {
#pragma unroll
                for (int q = 0; q < VEC; ++q) acc[q] = acc[q] + v[u][q];
            }
        }
    }
}
// the grid of the fold launch in the geometry g of the chunk pass: one lane group a split row, `tiles` feature tiles
inline dim3 long_grid(const PlanRows &r, const RowGeom &g, int tiles) {
    const int rows_per_block = (64 >> g.log2g) * g.waves;
    return dim3((unsigned)((r.n_long + rows_per_block - 1) / rows_per_block), (unsigned)tiles);
}

// acc[c] = Σ over the G lanes of the group, by the butterfly p[l] + p[l ^ m], m = G / 2 .. 1: the xor stays inside the group
template <int N>
__device__ __forceinline__ void group_sum(float acc[N], int G) {
    for (int m = G >> 1; m > 0; m >>= 1) {
#pragma unroll
        for (int c = 0; c < N; ++c) acc[c] = acc[c] + __shfl_xor(acc[c], m, 64);
    }
}

}  // namespace gnnmp
