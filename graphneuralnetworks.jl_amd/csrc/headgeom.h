// headgeom.h — which lanes hold one attention head: the one rule the one-pass attention forward (gat_fused.hip), its two pullbacks
// (gat_backward.hip, attn_backward.hip) and the three-pass GAT (attention.hip) share.  A forward and a pullback that disagreed on it
// would fail on odd head widths only.  Host only, no HIP: tests/c_harness/headgeom_check.cpp compiles it with plain g++.
#pragma once
#include <stdint.h>

namespace gnnmp {

// what the kernels get as `lph`: the lane count itself when it is a power of two, otherwise a code group_sum<0> (common.h) decodes
inline int lph_code(int lph, int log2g) {
    return (lph & (lph - 1)) == 0 ? lph : (0x10000 | (log2g << 8) | lph);
}

// a lane's `vec` features must lie inside one head: vec0 (what pick_vec / narrow_vec allowed) halved until it divides C
inline int head_vec(int64_t C, int vec0) {
    int vec = vec0;
    while (vec > 1 && (C % vec) != 0) vec >>= 1;
    return vec;
}

struct HeadGeom {
    int vec;          // features a lane holds
    int lanes;        // H*C / vec: lanes that hold one feature row
    int log2g;        // smallest lane group that holds them all (NOT pick_log2g: the head butterfly needs the whole row in one group)
    int lph;          // lanes that hold one head
    int lph_code;     // lph as the kernels take it
    bool fits_wave;   // lanes <= 64; the rest of the struct is for rows that do
};
inline HeadGeom head_geom(int64_t H, int64_t C, int vec0) {
    HeadGeom g;
    g.vec = head_vec(C, vec0);
    g.lanes = (int)(H * C / g.vec);
    g.log2g = 0;
    while ((1 << g.log2g) < g.lanes) ++g.log2g;
    g.fits_wave = g.lanes <= 64;
    g.lph = (int)(C / g.vec);
    if (H == 1 && g.fits_wave) g.lph = 1 << g.log2g;   // a single head may spill over idle lanes: they carry zeros
    g.lph_code = lph_code(g.lph, g.log2g);   // odd head widths (C = 7 classes, ...) sum their lanes one by one
    return g;
}

}  // namespace gnnmp
