// neighbors_grid.h — the host entry points of the cell-grid search (neighbors_grid.hip), called by threshold_graph in neighbors.hip
#pragma once
#include "common.h"
#include "neighbors_route.h"
#include "scratch.h"

#pragma GCC visibility push(hidden)
namespace gnnmp {

// the index of one call: the points binned by (graph, cell).  Scratch of the call, freed when it returns.
struct GridIndex {
    NbGrid geo;
    int64_t N = 0;
    DevBuf<uint32_t> keys;    // [N] sorted keys: graph * cells + (cz * ncy + cy) * ncx + cx; geo.table - 1 = in no cell (non-finite)
    DevBuf<uint32_t> start;   // [geo.table] first sorted position of every key
    DevBuf<float4> rec;       // [N] cell-ordered copy: (x, y, z, bits of j), a missing dimension is 0
};

// the box of the finite points and their count: one reduction kernel, read on the host (synchronises the stream)
int grid_bbox(const float *x, int64_t N, int d, hipStream_t stream, NbBox &box);
// keys, a stable sort of (key, j) (sort_scan.h: the members of a cell ascend in j), the cell-start table, the packed copy
int grid_build(GridIndex &ix, const NbGrid &geo, const float *x, int64_t N, int d, const void *gi, int gi_bytes, int base, hipStream_t stream);
// deg[i] = hits of centre i; *max_deg (zeroed by the caller) = the largest of them
int grid_count(const GridIndex &ix, float r2, int self_loops, int64_t *deg, int64_t *max_deg, hipStream_t stream);
// the hits of centre i into slots rowptr[i] ..., then every row put into ascending j (max_deg <= NB_GRID_ROW_CAP)
int grid_write(const GridIndex &ix, float r2, int self_loops, const int64_t *rowptr, int32_t *col, int32_t *eid, int64_t max_deg,
               hipStream_t stream);

}  // namespace gnnmp
#pragma GCC visibility pop
