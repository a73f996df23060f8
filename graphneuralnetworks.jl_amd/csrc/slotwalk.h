// slotwalk.h — the pieces every kernel shares that walks the rows of a plan WHOLE with one lane group a row: the training kernels of
// edge_conv.hip, cg_grad.hip, nn_grad.hip, egnn.hip, gmm.hip and megnet.hip, maxmin_grad.h and linkpred.hip's row_accumulate.
//
// What a whole-row walk is.  No atomics, no plan-owned scratch, every output element written exactly once (rows without in-edges and
// rows without out-edges included).  The kernels walk every row WHOLE, in slot order — original edge order — whatever its length: their
// PlanRows is plan_rows_whole's (no chunk virtual rows) and decode_vrow is told not to skip the rows longer than long_thresh
// (VROW_WHOLE).  Every sum therefore has the bits of the sequential fold and two calls give equal bits; the price is that A HUB ROW IS
// WALKED BY ONE LANE GROUP: correct, slow.  Chunked hub rows are a later change — and one that is made HERE and in the loops named
// below, not once per file.
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

// acc[c] = Σ over the G lanes of the group, by the butterfly p[l] + p[l ^ m], m = G / 2 .. 1: the xor stays inside the group
template <int N>
__device__ __forceinline__ void group_sum(float acc[N], int G) {
    for (int m = G >> 1; m > 0; m >>= 1) {
#pragma unroll
        for (int c = 0; c < N; ++c) acc[c] = acc[c] + __shfl_xor(acc[c], m, 64);
    }
}

}  // namespace gnnmp
