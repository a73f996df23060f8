// headgeom_check.cpp — CPU driver of csrc/headgeom.h: the SAME header the library compiles, under plain g++.  One line per case,
//   H C vec0 : vec lanes log2g lph lph_code fits_wave arm16 arm64
// arm16 / arm64: the LPH instance with_lph<vec, 16> / with_lph<vec, 64> (common.h) selects, restated here as plain integer code so that
// no HIP header is needed.  tests/test_headgeom_cpu.py compares every line with its own restatement of the rule.
#include <stdio.h>

#include "headgeom.h"

static int arm(int vec, int lph, int max) { return vec == 4 && lph >= 1 && lph <= max && (lph & (lph - 1)) == 0 ? lph : 0; }

int main() {
    const int Hs[] = {1, 2, 3, 4, 5, 6, 7, 8, 12, 16, 32, 64}, extraC[] = {96, 100, 128, 256}, vecs[] = {1, 2, 4};
    for (int H : Hs)
        for (int k = 1; k <= 84; ++k) {
            const int C = k <= 80 ? k : extraC[k - 81];
            for (int vec0 : vecs) {
                const gnnmp::HeadGeom g = gnnmp::head_geom(H, C, vec0);
                if (gnnmp::head_vec(C, vec0) != g.vec) return 1;
                printf("%d %d %d : %d %d %d %d %d %d %d %d\n", H, C, vec0, g.vec, g.lanes, g.log2g, g.lph, g.lph_code, g.fits_wave ? 1 : 0,
                       arm(g.vec, g.lph, 16), arm(g.vec, g.lph, 64));
            }
        }
    return 0;
}
