// grouped_route_check.cpp — CPU driver of csrc/dense_grouped_route.h: the SAME header the library compiles, under plain g++.  Reads one
// query per line from stdin,
//   N G K Dout x_al16 out_al16 want_dw cus
// and prints both planners' routes for it, one line of 16 integers in the order of tests/test_grouped_route_cpu.py: FIELDS:
//   kernel ncb waves tiles_per_block grid_x grid_y lds_bytes | g_kernel slabs g_waves tiles_per_wave g_grid_x g_grid_y g_grid_z fold_y
//   workspace
// (the forward route of the shape, then the weight-gradient route of the same shape with x_al16 as its one alignment fact).
#include <stdio.h>

#include "dense_grouped_route.h"

static_assert(gnnmp::grouped_t16_lds(20, 2) == 8 * 2 * 16 * 16 + 2 * 16 * 4 && gnnmp::grouped_t16_lds(1284, 2) > gnnmp::DENSE_LDS_BYTES,
              "the size function is a constant expression");

int main() {
    long long N, G, K, Dout;
    int xa, oa, want_dw, cus;
    long long lines = 0;
    while (scanf("%lld %lld %lld %lld %d %d %d %d", &N, &G, &K, &Dout, &xa, &oa, &want_dw, &cus) == 8) {
        const gnnmp::GroupedShape s{N, G, K, Dout, xa != 0, oa != 0};
        const gnnmp::GroupedRoute r = gnnmp::grouped_plan(s, cus);
        const gnnmp::GroupedGradRoute g = gnnmp::grouped_grad_plan(s, want_dw != 0, cus);
        printf("%d %d %d %lld %u %u %zu %d %d %d %d %u %u %u %u %lld\n", r.kernel, r.ncb, r.waves, (long long)r.tiles_per_block, r.grid_x,
               r.grid_y, r.lds_bytes, g.kernel, g.slabs, g.waves, g.tiles_per_wave, g.grid_x, g.grid_y, g.grid_z, g.fold_y,
               (long long)gnnmp::grouped_grad_workspace(N, G, Dout, K, cus));
        ++lines;
    }
    return lines > 0 ? 0 : 1;
}
