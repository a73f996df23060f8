// dense_route_check.cpp — CPU driver of csrc/dense_route.h: the SAME header the library compiles, under plain g++.  Reads one query
// per line from stdin,
//   N D1 D2 Dout x1_al16 x2_al16 out_al16 out_al128 cus generic split variant t16_waves prefetch
// and prints the planner's route for it, one line of 26 integers in the order of tests/dense_route_cases.py: FIELDS:
//   kernel tw waves ks tp rem_nt prefetch full ncb k0c k1c var maxb kq1 kq2 nout nt_full grid_x grid_y lds_bytes xld old region
//   ktot_pad skew token
// tests/test_dense_route_cpu.py feeds it the grid and compares every line with its own restatement of the parent's host paths.
#include <stdio.h>

#include "dense_route.h"

static_assert(gnnmp::split_img_bytes(208, 128) == 159744 && gnnmp::t16_img_rows(100) == 28 && gnnmp::split_threads(4, 4) == 768 &&
                  gnnmp::t16_max_threads(8) == 768,
              "the size functions are constant expressions");

int main() {
    long long N, D1, D2, Dout;
    int x1a, x2a, o16, o128, cus;
    gnnmp::DenseKnobs k{};
    long long lines = 0;
    while (scanf("%lld %lld %lld %lld %d %d %d %d %d %d %d %d %d %d", &N, &D1, &D2, &Dout, &x1a, &x2a, &o16, &o128, &cus, &k.generic,
                 &k.split, &k.variant, &k.t16_waves, &k.prefetch) == 14) {
        gnnmp::DenseShape s{};
        s.N = N; s.D1 = D1; s.D2 = D2; s.Dout = Dout;
        s.x1_al16 = x1a != 0; s.x2_al16 = x2a != 0; s.out_al16 = o16 != 0; s.out_al128 = o128 != 0;
        const gnnmp::DenseRoute r = gnnmp::dense_plan(s, k, cus);
        printf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %u %u %zu %d %d %d %d %d %d\n", r.kernel, r.tw, r.waves, r.ks, r.tp,
               r.rem_nt, r.prefetch, r.full, r.ncb, r.k0c, r.k1c, r.var, r.maxb, r.kq1, r.kq2, r.nout, r.nt_full, r.grid_x, r.grid_y,
               r.lds_bytes, r.xld, r.old_, r.region, r.ktot_pad, r.skew, r.token);
        ++lines;
    }
    return lines > 0 ? 0 : 1;
}
