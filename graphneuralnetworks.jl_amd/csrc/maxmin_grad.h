// maxmin_grad.h — the winners walk of the max / min adjoint, shared by maxmin_grad_kernel (backward.hip: one relation, split rows as
// chunks) and hetero_grad_rows_kernel (hetero_backward.hip: every relation that leaves a source row, the row walked whole).
//   acc[d] += Σ_{slots p in [beg, end)} (xv[d] == y[col_p][d]) ? dy[col_p][d] : 0      (ties: every maximiser gets Δ, like NNlib)
// in slot order — original edge order; U rows of y and of dy in flight per lane group.  All lanes of the group call this together.
#pragma once
#include "slotwalk.h"

namespace gnnmp {

template <int VEC, int U>
__device__ __forceinline__ void maxmin_grad_range(const int32_t *col, const float *y, const float *dy, int D, uint32_t beg, uint32_t end,
                                                  int lig, int gbase, int G, int f0, bool active, const float xv[VEC], float acc[VEC]) {
    for (uint32_t base = beg; base < end; base += G) {
        const Slots s = load_slots<true, false>(col, nullptr, base, end, lig, G);
        for (int j = 0; j < s.n; j += U) {
            float yv[U][VEC], dv[U][VEC];
            int cjs[U];
            bcast_word<U>(s.c, s.n, gbase, j, cjs);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int cj = cjs[u];
                if (active) {   // clamped, unconditional within the lane's activity: no per-element branch + wait
                    Vec<VEC>::load(y + (int64_t)cj * D + f0, yv[u]);
                    Vec<VEC>::load(dy + (int64_t)cj * D + f0, dv[u]);
                } else {
#pragma unroll
                    for (int q = 0; q < VEC; ++q) { yv[u][q] = 0.0f; dv[u][q] = 0.0f; }
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (j + u < s.n) {
#pragma unroll
                    for (int q = 0; q < VEC; ++q) acc[q] = acc[q] + (xv[q] == yv[u][q] ? dv[u][q] : 0.0f);
                }
            }
        }
    }
}

}  // namespace gnnmp
