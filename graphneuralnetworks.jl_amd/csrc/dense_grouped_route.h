// dense_grouped_route.h — which kernel a gnnmp_grouped_dense_f32 / gnnmp_grouped_dense_grad_w_f32 call reaches, which template instance of
// it and with what launch geometry: decided ONCE, on the host, as a value (the pattern of dense_route.h, whose size functions it uses).
// The exports of dense_grouped.hip validate, build a shape, call the planner here, keep the route in the calling thread's record
// (gnnmp_debug_grouped_dense_route) and launch what it names; the kernels decide nothing.  Plain C++17, no HIP header:
// tests/test_grouped_dense_abi.py compiles this file with g++.
//
// The group boundaries (seg_ptr) live on the device and are never read here: every geometry below is a function of N, G, K, Dout, the
// alignment of the operands and the CU count.  N / G — the mean group — is the only thing the host knows of the sizes.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "dense_route.h"

namespace gnnmp {

struct GroupedShape {
    int64_t N, G, K, Dout;     // validated by the export: N, G >= 0; 0 < K, Dout <= 2^20 (2^16 for the weight gradient)
    bool x_al16;               // x (dz and x for the gradient) is 16-byte aligned and its leading dimension a multiple of 4
    bool out_al16;             // the same for out (not looked at by the gradient)
};

enum GroupedKernel { GROUPED_NONE = 0, GROUPED_T16 = 1, GROUPED_FMA = 2, GROUPED_GRADW16 = 3, GROUPED_GRADW_FMA = 4 };

// ---- forward ---------------------------------------------------------------------------------------------------------------------------
struct GroupedRoute {
    int kernel;                // GroupedKernel; GROUPED_NONE = nothing to launch (N == 0)
    int ncb;                   // t16: column blocks of 16 a column tile: grouped_t16_kernel<NCB>
    int waves;                 // t16: waves a block; a super-tile is waves * 16 rows
    int64_t tiles_per_block;   // t16: super-tiles a block owns (a contiguous range); fma: rows a block owns
    unsigned grid_x, grid_y;
    size_t lds_bytes;          // t16: the W image of one group's column tile + its bias
};

constexpr size_t grouped_t16_lds(int K, int ncb) { return (size_t)t16_img_rows(K) * ncb * 16 * 16 + (size_t)ncb * 16 * 4; }

// the fp32 16x16x4 core takes whole float4 of rows that start on 16 bytes; the W image of a column tile must fit LDS.  Column blocks as
// plan_t16 picks them (as few padded columns as the shape allows), stepped down while the image of the tile does not fit.
inline int grouped_t16_ncb(const GroupedShape &s) {
    if ((s.K & 3) || (s.Dout & 3) || !s.x_al16 || !s.out_al16) return 0;
    const int64_t cb = (s.Dout + 15) / 16;
    const int first = cb >= 8 ? 8 : cb == 7 ? 7 : cb > 4 ? 6 : cb > 2 ? 4 : 2;
    for (int ncb : {8, 7, 6, 4, 2})
        if (ncb <= first && grouped_t16_lds((int)s.K, ncb) <= DENSE_LDS_BYTES) return ncb;
    return 0;
}

inline GroupedRoute grouped_plan(const GroupedShape &s, int cus) {
    GroupedRoute r{};
    if (s.N == 0) return r;
    const int ncb = grouped_t16_ncb(s);
    if (ncb == 0) {
        // lanes over the output columns of a block's rows: about 4 096 outputs a block
        r.kernel = GROUPED_FMA;
        r.tiles_per_block = std::max<int64_t>(1, std::min<int64_t>(256, 4096 / s.Dout));
        r.grid_x = (unsigned)((s.N + r.tiles_per_block - 1) / r.tiles_per_block);
        r.grid_y = 1;
        return r;
    }
    r.kernel = GROUPED_T16;
    r.ncb = ncb;
    r.lds_bytes = grouped_t16_lds((int)s.K, ncb);
    const int DP = ncb * 16;
    // Waves a block.  A super-tile that straddles group boundaries is walked once per group with the other groups' rows masked, so a
    // super-tile should not be much longer than the mean group; and like plan_t16 no more waves than the rows give every CU.
    const int64_t ntiles = (s.N + 15) / 16;
    const int max_waves = t16_max_threads(ncb) / 64;
    const int64_t mean = s.N / std::max<int64_t>(1, s.G);
    int64_t waves = std::min<int64_t>(max_waves, std::max<int64_t>(4, (ntiles + cus - 1) / cus));
    waves = std::min<int64_t>(waves, std::max<int64_t>(1, (mean + 15) / 16));
    r.waves = (int)waves;
    // Blocks: small blocks share a CU as far as LDS and the wave slots allow (at most 8); the super-tiles are dealt out in contiguous ranges
    const int64_t by_lds = (int64_t)(DENSE_LDS_BYTES / r.lds_bytes), by_waves = 32 / waves;
    const int64_t per_cu = std::max<int64_t>(1, std::min<int64_t>(8, std::min(by_lds, by_waves)));
    const int64_t nst = (ntiles + waves - 1) / waves;
    const int64_t blocks = std::min<int64_t>(nst, per_cu * cus);
    r.tiles_per_block = (nst + blocks - 1) / blocks;
    r.grid_x = (unsigned)((nst + r.tiles_per_block - 1) / r.tiles_per_block);
    r.grid_y = (unsigned)((s.Dout + DP - 1) / DP);
    return r;
}

// ---- the weight gradient ----------------------------------------------------------------------------------------------------------------
struct GroupedGradRoute {
    int kernel;                // GROUPED_GRADW16 | GROUPED_GRADW_FMA (never NONE: empty groups are written as zeros)
    int slabs;                 // S: slabs a group, the same for every group; block b reduces slab b % S of group b / S
    int waves;                 // gradw16: waves a block (they split the columns of dW)
    int tiles_per_wave;        // gradw16: 16-column tiles of dW a wave
    unsigned grid_x, grid_y, grid_z;
    unsigned fold_y;           // the fold launch: grid (G (+ 1 for a shared db), fold_y)
};

// S from the mean group and the CU count: G * S blocks fill the chip about twice, a slab holds at least 64 rows of the mean group
inline int grouped_grad_slabs(int64_t N, int64_t G, int cus) {
    if (G <= 0) return 1;
    const int64_t want = (2 * (int64_t)cus + G - 1) / G;
    const int64_t by_rows = std::max<int64_t>(1, (N / G) / 64);
    return (int)std::max<int64_t>(1, std::min<int64_t>(std::min(want, by_rows), 1024));
}
// floats of the caller's workspace: the slabs' private dW partials, then their db partials
inline int64_t grouped_grad_workspace(int64_t N, int64_t G, int64_t Dout, int64_t K, int cus) {
    if (G <= 0 || Dout <= 0 || K <= 0) return 0;
    return G * grouped_grad_slabs(N, G, cus) * (Dout * K + Dout);
}

inline GroupedGradRoute grouped_grad_plan(const GroupedShape &s, bool want_dw, int cus) {
    GroupedGradRoute r{};
    r.slabs = grouped_grad_slabs(s.N, s.G, cus);
    r.grid_x = (unsigned)(s.G * r.slabs);
    const int64_t len = (want_dw ? s.Dout * s.K : 0) + s.Dout;
    r.fold_y = (unsigned)std::max<int64_t>(1, std::min<int64_t>(1024, (len + 255) / 256));
    if (want_dw && !(s.K & 3) && !(s.Dout & 3) && s.x_al16) {
        // dense_gradw16_kernel's split: a wave owns up to 8 x 4 tiles of 16 x 16, the waves of a block share the dz rows
        r.kernel = GROUPED_GRADW16;
        const int ktiles = (int)((s.K + 15) / 16);
        const int kwaves_all = (ktiles + 3) / 4;
        r.waves = std::min(4, kwaves_all);
        const int kblocks = (kwaves_all + r.waves - 1) / r.waves;
        r.tiles_per_wave = (ktiles + kblocks * r.waves - 1) / (kblocks * r.waves);
        r.grid_y = (unsigned)((s.Dout + 127) / 128);
        r.grid_z = (unsigned)kblocks;
        return r;
    }
    r.kernel = GROUPED_GRADW_FMA;
    r.grid_y = (unsigned)std::max<int64_t>(1, std::min<int64_t>(64, (len + 255) / 256));
    r.grid_z = 1;
    return r;
}

}  // namespace gnnmp
