// rowwalk.h — the ONE place the virtual-row convention of the aggregation kernels is defined: the device view of a plan's row
// structure (PlanRows), the launch geometry of a row walk (RowGeom, row_grid) and the decode every row kernel starts with
// (decode_vrow).
//
// Virtual rows: [0, n_chunks) are the chunks of the rows the plan splits (longer than long_thresh; plan.hip cuts them into balanced
// chunks of at most long_thresh slots), [n_chunks, n_chunks + n_rows) the ordinary rows.  A lane group of G = 2^log2g lanes takes one
// virtual row; an ordinary row longer than long_thresh is skipped because its chunks stand in for it (their partials are folded by
// the kernel's combine step).  The dominant kernel therefore touches every edge exactly once and has no tail.
#pragma once
#include <algorithm>
#include <initializer_list>

#include "common.h"

namespace gnnmp {

// Slots are UNSIGNED 32-bit (a plan holds fewer than 2^32 - 65536 of them): the walk costs what it cost with int32 slots.
// (A 64-bit rowptr was tried first: 64-bit loop counters cost the VALU-sensitive attention kernel 7 % on the products shape,
// and with per-row base pointers instead the row kernels went from 78 to 90 VGPRs — 6 -> 5 waves per SIMD, arxiv shape +4 %.)
// The ORDER of the fields is deliberate: the first eleven are the adjoint kernels' old argument prefix.  With the later additions in
// front of the chunk tables gat_bwd_src_kernel<4, 8, .> went from 95 to 127 VGPRs on identical IR (the machine scheduler follows the
// SGPR pressure the kernarg loads leave behind: LABNOTES.md, 2026-10-18) — compare the code objects' notes before reordering.
struct PlanRows {
    const uint32_t *rowptr;      // [n_rows + 1]
    const int32_t *col;          // per slot: the row to gather (plan->col; the scatter kernels walk plan->eid here instead)
    const int32_t *chunk_row;    // [n_chunks] the row a chunk belongs to
    const uint32_t *chunk_beg, *chunk_end;
    const int32_t *long_rows;    // [n_long] the split rows, ascending
    const int32_t *long_cptr;    // [n_long + 1] chunk range of each split row
    int n_chunks, n_long, n_rows, long_thresh;
    const int32_t *eid;          // per slot: original edge position, to be read as unsigned 32 bits
    const int32_t *row_order;    // [n_rows] rows by decreasing length, or null (common.h: gnnmp_graph::row_order, use_row_order)
    const int32_t *chunk_lrow;   // [n_chunks] chunk_row as an index into long_rows (fold-in-kernel: csr_reduce.h long_geom)
    uint32_t n_edges;            // per-edge operands exist for eid < n_edges; plan-added self loops lie beyond
};

// Everything a plan says about its rows.  What a call chooses — eid for col, n_rows = 0 for a chunks-only pass, row_order when
// use_row_order says so — is an explicit override of the returned value at the call site.
inline PlanRows plan_rows(const gnnmp_graph *p) {
    PlanRows r;
    r.rowptr = p->rowptr;
    r.col = p->col;
    r.eid = p->eid;
    r.row_order = nullptr;
    r.chunk_row = p->chunk_row;
    r.chunk_beg = p->chunk_beg;
    r.chunk_end = p->chunk_end;
    r.chunk_lrow = p->chunk_lrow;
    r.long_rows = p->long_rows;
    r.long_cptr = p->long_cptr;
    r.n_rows = (int)p->n_dst;
    r.n_chunks = p->n_chunks;
    r.n_long = p->n_long;
    r.long_thresh = p->long_thresh;
    r.n_edges = (uint32_t)p->n_edges;
    return r;
}
// The view of a kernel that walks every row WHOLE (decode_vrow<VROW_WHOLE>; slotwalk.h says what that buys and costs): no chunk virtual
// rows, so the rows longer than long_thresh are walked themselves.
inline PlanRows plan_rows_whole(const gnnmp_graph *p) {
    PlanRows r = plan_rows(p);
    r.n_chunks = 0;
    r.n_long = 0;
    return r;
}

struct RowGeom {
    int log2g;   // lanes per virtual row = 1 << log2g
    int waves;   // waves per block
    int cpx;     // logical blocks per XCD (grid.x = nbc + 8 * cpx); 0 = no remap
    int nbc;     // leading blocks (chunk virtual rows) that are not remapped (common.h: xcd_remap_after)
};

// blocks of (64 >> log2g) * waves virtual rows that cover the plan
inline int64_t row_blocks(const PlanRows &r, const RowGeom &g) {
    const int rows_per_block = (64 >> g.log2g) * g.waves;
    return ((int64_t)r.n_rows + r.n_chunks + rows_per_block - 1) / rows_per_block;
}
// the grid of a row walk over `tiles` feature tiles; sets g.cpx / g.nbc (remap: the caller's use_xcd_remap verdict).  grid.x == 0: no rows.
inline dim3 row_grid(const PlanRows &r, RowGeom &g, int tiles, bool remap = false) {
    const int rows_per_block = (64 >> g.log2g) * g.waves;
    const int64_t blocks = row_blocks(r, g);
    int64_t gx = blocks;
    g.cpx = 0;
    g.nbc = 0;
    if (remap) {
        g.nbc = (int)std::min<int64_t>(blocks, (r.n_chunks + rows_per_block - 1) / rows_per_block);
        g.cpx = (int)((blocks - g.nbc + 7) / 8);
        gx = (int64_t)g.nbc + (int64_t)g.cpx * 8;
    }
    return dim3((unsigned)gx, (unsigned)tiles);
}
// row_grid for an export that chose g.log2g / g.waves itself, or the refusal of a plan with more row blocks than a grid holds
inline int row_walk_grid(const char *who, const PlanRows &r, RowGeom &g, int tiles, dim3 &grid) {
    if (row_blocks(r, g) >= INT32_MAX) return fail(GNNMP_EUNSUPPORTED, "%s: too many row blocks", who);
    grid = row_grid(r, g, tiles);
    return GNNMP_OK;
}
// The geometry of a row walk with one lane group a row and vec floats of `width` a lane.  Returns vec — the widest Vec<vec> access
// that every array of `arrays` admits (a null one admits any) — or a failure (< 0); fills g (4 waves a block) and the grid over `tiles`
// feature tiles (0: feature_tiles of the width).  Column k * width inside a row (the planar [n][2C] and [n][K C] matrices) needs no
// entry of its own: width % vec == 0, so it is aligned whenever the row is.  align_extra: further bits that must be aligned like the
// pointers — the byte row strides of arrays whose rows are not `width` apart (the panel hop).
inline int row_walk_geom(const char *who, const PlanRows &r, int64_t width, int tiles, std::initializer_list<const float *> arrays,
                         RowGeom &g, dim3 &grid, uintptr_t align_extra = 0) {
    uintptr_t align = align_extra;
    for (const float *p : arrays) align |= reinterpret_cast<uintptr_t>(p);
    const int vec = pick_vec(width, reinterpret_cast<const void *>(align), nullptr);
    g = RowGeom{pick_log2g((width + vec - 1) / vec), 4, 0, 0};
    const int rc = row_walk_grid(who, r, g, tiles ? tiles : feature_tiles(width, vec, g.log2g), grid);
    return rc != GNNMP_OK ? rc : vec;
}

struct VRow {
    int v;            // virtual row
    bool is_chunk;
    int row;          // the destination (of the chunk, or the row itself)
    uint32_t beg, end;
    int lig, gbase, G;   // lane in group, first lane of the group, lanes per group
};

// The virtual row of the calling lane group in (logical) block `block`; false = nothing to do (past the last virtual row, or the
// slot of a split row).  What only some kernels need is a compile-time flag, so that the others carry no trace of it:
//   VROW_REMAP         the host side may set g.cpx (XCD-contiguous blocks)
//   VROW_ORDER         the host side may set r.row_order
//   VROW_NO_CHUNK_ROW  the kernel never reads .row of a chunk: skip the chunk_row lookup (.row = 0 there).  The compiler does not
//                      drop that load by itself — .row merges with the ordinary rows' before the kernel tells the two apart again.
//   VROW_WHOLE         the kernel walks every ordinary row whole, whatever its length (its PlanRows carries n_chunks = 0): a row
//                      longer than long_thresh is NOT skipped
enum { VROW_REMAP = 1, VROW_ORDER = 2, VROW_NO_CHUNK_ROW = 4, VROW_WHOLE = 8 };
template <int FLAGS = 0>
__device__ __forceinline__ bool decode_vrow(const PlanRows &r, const RowGeom &g, int block, VRow &w) {
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    w.G = 1 << g.log2g;
    w.lig = lane & (w.G - 1);
    w.gbase = lane - w.lig;
    const int grp = lane >> g.log2g;
    const int rpw = 64 >> g.log2g;
    if ((FLAGS & VROW_REMAP) && g.cpx) block = xcd_remap_after(block, g.nbc, g.cpx);
    const int64_t v64 = ((int64_t)block * g.waves + wave) * rpw + grp;
    if (v64 >= (int64_t)r.n_rows + r.n_chunks) return false;
    w.v = (int)v64;
    w.is_chunk = w.v < r.n_chunks;
    if (w.is_chunk) {
        w.row = (FLAGS & VROW_NO_CHUNK_ROW) ? 0 : r.chunk_row[w.v];
        w.beg = r.chunk_beg[w.v];
        w.end = r.chunk_end[w.v];
    } else {
        w.row = w.v - r.n_chunks;
        if ((FLAGS & VROW_ORDER) && r.row_order) w.row = r.row_order[w.row];
        w.beg = r.rowptr[w.row];
        w.end = r.rowptr[w.row + 1];
        if (!(FLAGS & VROW_WHOLE) && w.end - w.beg > (uint32_t)r.long_thresh) return false;   // split row: its chunks are virtual rows
    }
    return true;
}

}  // namespace gnnmp
