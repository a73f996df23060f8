// headtiles_check.cpp — CPU driver of csrc/headgeom.h's head_tiles: the SAME header the library compiles, under plain g++.  For every
// "H C vec0" triple of the command line one line:  vec lph lph_code hpt tiles fits   (tests/test_attn_wide.py compares them with its table)
#include <stdio.h>
#include <stdlib.h>

#include "headgeom.h"

int main(int argc, char **argv) {
    for (int k = 1; k + 2 < argc; k += 3) {
        const gnnmp::HeadTiles t = gnnmp::head_tiles(atol(argv[k]), atol(argv[k + 1]), atoi(argv[k + 2]));
        printf("%d %d %d %d %d %d\n", t.vec, t.lph, t.lph_code, t.hpt, t.tiles, t.fits ? 1 : 0);
    }
    return 0;
}
