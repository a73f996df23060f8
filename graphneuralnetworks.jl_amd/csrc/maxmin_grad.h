// maxmin_grad.h — the winners walk of the max / min adjoint, shared by maxmin_grad_kernel (backward.hip: one relation, split rows as
// chunks) and hetero_grad_rows_kernel (hetero_backward.hip: every relation that leaves a source row, the row walked whole).
//   acc[d] += Σ_{slots p in [beg, end)} (xv[d] == y[col_p][d]) ? dy[col_p][d] : 0      (ties: every maximiser gets Δ, like NNlib)
// in slot order — original edge order; U rows of y and of dy in flight per lane group.  All lanes of the group call this together.
#pragma once
#include "common.h"

namespace gnnmp {

template <int VEC, int U>
__device__ __forceinline__ void maxmin_grad_range(const int32_t *col, const float *y, const float *dy, int D, uint32_t beg, uint32_t end,
                                                  int lig, int gbase, int G, int f0, bool active, const float xv[VEC], float acc[VEC]) {
    for (uint32_t base = beg; base < end; base += G) {   // slots are unsigned 32-bit (rowwalk.h)
        const uint32_t p = base + lig;
        const int c = p < end ? col[p] : 0;
        const int n = (int)min((uint32_t)G, end - base);
        for (int j = 0; j < n; j += U) {
            float yv[U][VEC], dv[U][VEC];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int cj = __shfl(c, gbase + min(j + u, n - 1), 64);
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
                if (j + u < n) {
#pragma unroll
                    for (int q = 0; q < VEC; ++q) acc[q] = acc[q] + (xv[q] == yv[u][q] ? dv[u][q] : 0.0f);
                }
            }
        }
    }
}

}  // namespace gnnmp
