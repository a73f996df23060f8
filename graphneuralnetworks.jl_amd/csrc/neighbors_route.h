// neighbors_route.h — which search a gnnmp_radius_graph_f32 call runs and, for the cell grid, its geometry: decided ONCE, on the host, as a
// value (the pattern of dense_route.h and dense_grouped_route.h).  The export in neighbors.hip validates, fills a shape, asks the two
// functions here, keeps the answer in the calling thread's record (gnnmp_debug_neighbors_route) and launches what it names; the kernels
// of neighbors_grid.hip decide nothing.  Plain C++17, no HIP header: tests/test_neighbors_grid.py compiles this file with g++.
//
// Why a grid may replace the brute search bit for bit.  The semantics (gnnmp.h) make the answer unique, so a spatial index is a pure
// route as long as it never loses a hit.  It does not, by this argument (u = 2^-24, r the caller's radius, r2 = fl(r * r) finite):
//   (1) the chain acc_c = fl(D_c^2 + acc_{c-1}), D_c = fl(x_i[c] - x_j[c]), only grows (rounding is monotone, every term is >= 0), so a
//       hit d2 <= r2 has fl(D_c^2) <= r2 on every axis.  With r >= 2^-60 the square r * r is a normal number, r2 <= r^2 (1 + u), and
//       either D_c^2 < 2^-126 (then |D_c| < 2^-63 < r) or D_c^2 <= fl(D_c^2) (1 + u): |D_c| <= r (1 + u).  A subtraction that is exact
//       or rounded once gives |x_i[c] - x_j[c]| <= |D_c| (1 + u) <= r (1 + 2^-22) < r (1 + 2^-20).
//       A radius below 2^-60 (r = 0 included) is planned as 2^-60: the bound above then holds with 2^-60 in the place of r.
//   (2) the cell side is h >= max(r, 2^-60) (1 + 2^-10), so that distance is at most h (1 - 2^-11) — strictly inside one cell side.
//   (3) the cell coordinate is floor((double(x) - double(lo)) / h), clamped to the axis.  Two correctly rounded double operations are
//       monotone in x, and their value u(x) carries a relative error below 2^-51; the table bound below keeps u(x) < 2^31, so the
//       absolute error is below 2^-20 cells.  Hence |u(x_i) - u(x_j)| <= 1 - 2^-11 + 2^-19 < 1 and the floors differ by at most one:
//       a hit lies within +-1 cell per axis.  Clamping is monotone and contracts differences, so it keeps that.
// The search therefore tests, for every centre, each point of the 3^d cells around its own exactly once with the brute kernel's fma
// chain; what it finds is what the brute kernel finds, and the row-order pass restores "neighbours ascend in j".
// r2 = +inf (r * r overflows) is outside the argument — the brute rule then takes EVERY candidate, non-finite ones included — and is
// one of the reasons below.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>

namespace gnnmp {

enum NbRouteKind { NB_ROUTE_NONE = 0, NB_ROUTE_BRUTE = 1, NB_ROUTE_GRID = 2, NB_ROUTE_GRID_COUNT_BRUTE_WRITE = 3 };
enum NbForce { NB_FORCE_AUTO = 0, NB_FORCE_BRUTE = 1, NB_FORCE_GRID = 2 };
// why a call did not take (all of) the grid: info[5] of gnnmp_debug_neighbors_route
enum NbWhy {
    NB_WHY_NONE = 0,
    NB_WHY_DIM = 1,          // d > 3
    NB_WHY_UNSORTED = 2,     // the indicator decreases somewhere
    NB_WHY_R2_INF = 3,       // r * r overflows fp32: every candidate is a neighbour, there is nothing to prune
    NB_WHY_N_RANGE = 4,      // N == 0, or N above NB_GRID_MAX_N (the keys are 32-bit)
    NB_WHY_GRAPHS = 5,       // more graphs than the table has cells
    NB_WHY_SMALL = 6,        // auto: below the measured crossover
    NB_WHY_FEW_CELLS = 7,    // auto: the box is only a few cutoffs wide, the 3^d neighbourhood is most of it
    NB_WHY_FORCED_BRUTE = 8,
    NB_WHY_ROW_CAP = 9,      // a row longer than NB_GRID_ROW_CAP: the grid counted, the brute kernel wrote (route 3)
    NB_WHY_METRIC = 10       // gnnmp_hyperbolic_graph_f32 has no grid
};

constexpr double NB_GRID_SLACK = 1.0 + 1.0 / 1024.0;   // h >= r (1 + 2^-10)
constexpr double NB_GRID_MIN_R = 0x1p-60;
// The cell-start table holds graphs x cells + 1 entries and is sized from N alone, a LINEAR bound: at most 2 N + 4096 entries.  h grows
// until the cells fit, so a sparse cloud (or one outlier at 1e30) costs pruning, never memory.
constexpr int64_t NB_GRID_TABLE_PER_POINT = 2, NB_GRID_TABLE_MIN = 4096;
constexpr int64_t NB_GRID_MAX_N = (int64_t)1 << 29;    // keys < 2^30 + 4096 fit 32 bits with the sentinel
// rows the row-order kernel sorts (one lane group a row, the row in LDS); a longer row anywhere sends the WRITE pass to the brute kernel
constexpr int NB_GRID_ROW_CAP = 1024;
// The auto rule.  Work model: brute tests N * (N / G) pairs; the grid tests N * 3^d * (points a cell) * (1 + walk overhead) and pays a
// radix sort of N keys, one more host synchronisation and five small launches — a fixed cost of some hundred microseconds that a 1024-
// point cloud (10^6 pair tests, microseconds of brute work) can never earn back.  Measured ("Neighbour search: the two
// routes"; single clouds, d = 2 and 3, uniform and clustered, 16 and 64 neighbours): at 2^14 points the grid is 1.2-2.0x faster with a
// round-to-round spread of up to 8 % — too close to call on the worst row; at 2^15 it is 2.5-5.0x, at 2^17 17-43x, at 2^20 330-415x,
// and it loses on no measured row.  The crossover sits at 2^15.  Batched clouds were not measured: the rule asks the MEAN graph to
// offer the brute work of such a cloud.
constexpr int64_t NB_GRID_MIN_N = 32768;           // points of the call
constexpr int64_t NB_GRID_MIN_MEAN_GRAPH = 32768;  // N / G: the brute work a centre has to offer
constexpr int64_t NB_GRID_MIN_PRUNE = 4;           // cells of a graph >= this many 3^d neighbourhoods

inline int64_t nb_grid_table(int64_t N) { return NB_GRID_TABLE_PER_POINT * N + NB_GRID_TABLE_MIN; }

struct NbShape {
    int64_t N, d, G;       // G = 1 without an indicator
    float r;
    bool sorted;           // the indicator is absent or non-decreasing
    bool euclid;           // gnnmp_radius_graph_f32 (not the hyperbolic metric)
    int force;             // NbForce
};

struct NbBox {             // of the FINITE points (a point with a non-finite coordinate is in no cell)
    double lo[3], hi[3];
    int64_t n_finite;
};

struct NbGrid {
    int route;             // NB_ROUTE_BRUTE | NB_ROUTE_GRID
    int why;               // NbWhy when the route is brute
    double origin[3], h;
    int nc[3];             // cells per axis (1 on an axis the points do not have)
    int64_t cells;         // of one graph: nc[0] * nc[1] * nc[2]
    int64_t table;         // G * cells + 1 entries of the cell-start table; key G * cells = "no cell"
};

// Step 1, before anything is launched: may the call take the grid at all?  NB_WHY_NONE = go on to the bounding box.  A forced grid that
// gets another answer is refused by the export (GNNMP_EUNSUPPORTED); on auto it is today's brute search, untouched.
inline int nb_cheap_test(const NbShape &s) {
    if (s.force == NB_FORCE_BRUTE) return NB_WHY_FORCED_BRUTE;
    if (!s.euclid) return NB_WHY_METRIC;
    if (s.d > 3) return NB_WHY_DIM;
    if (!s.sorted) return NB_WHY_UNSORTED;
    if (s.N <= 0 || s.N > NB_GRID_MAX_N) return NB_WHY_N_RANGE;
    if (!(s.r * s.r < INFINITY)) return NB_WHY_R2_INF;
    if (s.G > nb_grid_table(s.N) - 1) return NB_WHY_GRAPHS;
    if (s.force == NB_FORCE_AUTO && (s.N < NB_GRID_MIN_N || s.N / std::max<int64_t>(s.G, 1) < NB_GRID_MIN_MEAN_GRAPH)) return NB_WHY_SMALL;
    return NB_WHY_NONE;
}

// cells of one graph at side h, as a double (1e30 / 1e-18 cubed is still a double)
inline double nb_cells_at(const NbShape &s, const NbBox &b, double h) {
    double c = 1.0;
    for (int a = 0; a < (int)s.d; ++a) c *= std::floor((b.hi[a] - b.lo[a]) / h) + 1.0;
    return c;
}

// Step 3, after the bounding box: the geometry.  Always a valid grid (one cell when r exceeds the extent, when the extent is zero, when
// no point is finite); on auto a grid that cannot prune goes back to brute.
inline NbGrid nb_plan_grid(const NbShape &s, const NbBox &box) {
    NbGrid g{};
    NbBox b = box;
    if (b.n_finite <= 0)
        for (int a = 0; a < 3; ++a) b.lo[a] = b.hi[a] = 0.0;
    const double budget = (double)((nb_grid_table(s.N) - 1) / std::max<int64_t>(s.G, 1));   // cells a graph may have (>= 1: nb_cheap_test)
    double h = std::max((double)s.r, NB_GRID_MIN_R) * NB_GRID_SLACK;
    if (nb_cells_at(s, b, h) > budget) {
        double bad = h;
        while (nb_cells_at(s, b, h) > budget) {   // (at most ~320 doublings: the extent is below 2^129, h at least 2^-60)
            bad = h;
            h *= 2.0;
        }
        for (int it = 0; it < 8; ++it) {          // the smallest side that fits, to 2^-8 of it
            const double mid = 0.5 * (bad + h);
            if (nb_cells_at(s, b, mid) > budget) bad = mid; else h = mid;
        }
    }
    g.h = h;
    g.cells = 1;
    int64_t hood = 1;
    for (int a = 0; a < 3; ++a) {
        g.origin[a] = a < (int)s.d ? b.lo[a] : 0.0;
        g.nc[a] = a < (int)s.d ? (int)(std::floor((b.hi[a] - b.lo[a]) / h) + 1.0) : 1;
        g.cells *= g.nc[a];
        hood *= std::min(g.nc[a], 3);
    }
    g.table = std::max<int64_t>(s.G, 1) * g.cells + 1;
    g.route = NB_ROUTE_GRID;
    if (s.force == NB_FORCE_AUTO && g.cells < NB_GRID_MIN_PRUNE * hood) {
        g.route = NB_ROUTE_BRUTE;
        g.why = NB_WHY_FEW_CELLS;
    }
    return g;
}

}  // namespace gnnmp
