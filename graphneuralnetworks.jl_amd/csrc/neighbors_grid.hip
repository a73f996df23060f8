// neighbors_grid.hip — the cell-grid route of radius_graph for d <= 3: the same plan as the brute search of neighbors.hip, bit for bit, in
// work N * 3^d * (points a cell) instead of sum n_g^2.  neighbors_route.h decides whether a call comes here and with what geometry, and
// holds the proof that no hit is lost; gnnmp.h states the semantics both routes share.
//
// Binning.  A point's key is graph * cells + (cz * ncy + cy) * ncx + cx, its cell coordinates computed in double; a point with a
// non-finite coordinate gets the key past the last cell and is a candidate of nobody, itself included (its d2 is non-finite against
// everyone).  (key, j) is sorted stably (sort_scan.h), so the members of a cell ascend in j; a binary search per cell writes the cell-start
// table; a cell-ordered copy packs a point as float4(x, y, z, bits of j): a candidate is ONE 16-byte load, and a dimension the points do
// not have is 0 on both sides — fmaf(0, 0, acc) == acc, so the chain's bits are those of the d-term chain.
//
// Search.  Centres are walked in CELL order: a workgroup is one wave and owns 64 consecutive sorted positions — a run of home cells (a
// dozen at the 4-5 points a cell of a 20-neighbour cutoff), whose 3^d neighbourhoods overlap almost entirely.  A lane owns a centre and
// keeps its record in registers.  The wave takes the x-rows of cells its centres sit in one at a time (usually one, two where the run
// crosses a row end): for a row piece with cells cxa .. cxb, the candidates are, for each of the 3 x 3 (dz, dy) neighbour rows that
// exist, the cells cxa - 1 .. cxb + 1 — ONE contiguous run of the sorted copy each, because cx is the fastest key digit: 9 runs in 3-D,
// 3 in 2-D, 1 in 1-D.  A run goes through LDS in tiles of 64 records (one coalesced 1 KB load, the next tile's records already in
// flight in registers); every lane then reads the tile record by record — a same-address ds_read_b128 is a broadcast — and evaluates
// acc = fmaf(xi - xj, xi - xj, acc) in the header's operand order: 3 subtractions, 3 fmas, 2 compares and an add a pair, against one LDS
// read.  Only the lanes of the row piece count what they see; every candidate of a piece is met exactly once, so the exact test alone
// decides (a superset of the 3^d cells costs time, never a duplicate).
//   count pass   hits per centre -> deg[j of the centre]; the largest degree by an integer max
//   write pass   the same walk, hits into the row's slots in WALK order, eid[e] = e
//   row order    one lane group a row: the row into LDS, every entry's rank = the entries below it (the j of a row are distinct), back in
//                ascending j.  16 lanes a row while the longest row is at most 64, a wave a row up to NB_GRID_ROW_CAP = 1024.
// No floating-point atomics; the integer min / max / add of the bounding box and the largest degree do not depend on the order.  Reruns
// are bit-identical.
#include <algorithm>
#include <cmath>

#include "neighbors_grid.h"
#include "sort_scan.h"

namespace gnnmp {
namespace {

constexpr int GS_TILE = 64;   // records a tile = lanes of the wave

struct GridGeoDev {
    double o[3], h;
    int nc[3];
    uint32_t cells, none;     // cells of one graph; the key of "no cell" (= graphs * cells)
};

// fp32 -> unsigned with the same order (-0 below +0); the box is reduced with integer min / max
__host__ __device__ inline uint32_t ord_enc(float f) {
    uint32_t u;
    __builtin_memcpy(&u, &f, 4);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
inline float ord_dec(uint32_t u) {
    u = (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u;
    float f;
    __builtin_memcpy(&f, &u, 4);
    return f;
}

struct GridStats {
    uint32_t lo[3], hi[3];
    unsigned long long n_finite;
};

__global__ void grid_stats_init_kernel(GridStats *s) {
    if (threadIdx.x < 3) {
        s->lo[threadIdx.x] = 0xffffffffu;
        s->hi[threadIdx.x] = 0u;
    }
    if (threadIdx.x == 0) s->n_finite = 0ULL;
}

__device__ __forceinline__ bool point_finite(const float *x, int64_t i, int d) {
    bool fin = true;
    for (int c = 0; c < d; ++c) {
        const float v = x[i * d + c];
        fin = fin && (v - v == 0.0f);
    }
    return fin;
}

__global__ void __launch_bounds__(256) grid_bbox_kernel(const float *x, int64_t N, int d, GridStats *s) {
    uint32_t lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u};
    unsigned long long n = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < N; i += (int64_t)gridDim.x * 256) {
        if (!point_finite(x, i, d)) continue;
        ++n;
        for (int c = 0; c < d; ++c) {
            const uint32_t e = ord_enc(x[i * d + c]);
            lo[c] = min(lo[c], e);
            hi[c] = max(hi[c], e);
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            lo[c] = min(lo[c], (uint32_t)__shfl_xor((int)lo[c], o, 64));
            hi[c] = max(hi[c], (uint32_t)__shfl_xor((int)hi[c], o, 64));
        }
        n += __shfl_xor(n, o, 64);
    }
    if ((threadIdx.x & 63) == 0 && n) {
        for (int c = 0; c < d; ++c) {
            atomicMin(&s->lo[c], lo[c]);
            atomicMax(&s->hi[c], hi[c]);
        }
        atomicAdd(&s->n_finite, n);
    }
}

__global__ void __launch_bounds__(256) grid_key_kernel(const float *x, int64_t N, int d, const void *gi, int gi_bytes, int base,
                                                       const GridGeoDev g, uint32_t *keys, uint32_t *vals) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    uint32_t key = g.none;
    if (point_finite(x, i, d)) {
        uint32_t cc[3] = {0u, 0u, 0u};
        for (int c = 0; c < d; ++c) {
            // floor((double(x) - double(lo)) / h): two correctly rounded, monotone operations (neighbors_route.h, step 3 of the argument)
            double u = floor(((double)x[i * d + c] - g.o[c]) / g.h);
            u = fmin(fmax(u, 0.0), (double)(g.nc[c] - 1));
            cc[c] = (uint32_t)u;
        }
        const uint32_t gr = gi ? (uint32_t)load_index(gi, i, gi_bytes, base) : 0u;
        key = gr * g.cells + (cc[2] * (uint32_t)g.nc[1] + cc[1]) * (uint32_t)g.nc[0] + cc[0];
    }
    keys[i] = key;
    vals[i] = (uint32_t)i;
}

// start[k] = the first sorted position whose key is >= k, for k = 0 .. table - 1 (the last entry: the number of points that have a cell)
__global__ void __launch_bounds__(256) grid_cell_start_kernel(const uint32_t *keys, int64_t N, int64_t table, uint32_t *start) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= table) return;
    int64_t lo = 0, hi = N;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t)keys[mid] < k) lo = mid + 1; else hi = mid;
    }
    start[k] = (uint32_t)lo;
}

__global__ void __launch_bounds__(256) grid_pack_kernel(const float *x, int64_t N, int d, const uint32_t *order, float4 *rec) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= N) return;
    const uint32_t j = order[p];
    float4 r;
    r.x = x[(int64_t)j * d];
    r.y = d > 1 ? x[(int64_t)j * d + 1] : 0.0f;
    r.z = d > 2 ? x[(int64_t)j * d + 2] : 0.0f;
    r.w = __uint_as_float(j);
    rec[p] = r;
}

enum { GS_COUNT = 0, GS_WRITE = 1 };

struct GridSearchArgs {
    const uint32_t *keys, *start;
    const float4 *rec;
    int64_t N;
    int ncx, ncy, ncz;
    uint32_t cells, none;
    float r2;
    int self_loops;
    int64_t *deg;                    // count
    unsigned long long *max_deg;     // count
    const int64_t *rowptr;           // write
    int32_t *col, *eid;              // write
};

template <int MODE>
__global__ void __launch_bounds__(64) grid_search_kernel(const GridSearchArgs a) {
    __shared__ float4 tile[GS_TILE];
    const int lane = threadIdx.x;
    const int64_t p = (int64_t)blockIdx.x * GS_TILE + lane;
    const bool in = p < a.N;
    const uint32_t key = in ? a.keys[p] : a.none;
    const bool live = key != a.none;
    const float4 me = in ? a.rec[p] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const uint32_t i = __float_as_uint(me.w);
    // the centre's x-row of cells (graph and (cz, cy) in one number: key / ncx) and its place in it
    const uint32_t rowkey = key / (uint32_t)a.ncx;
    const int cx = (int)(key - rowkey * (uint32_t)a.ncx);
    const uint32_t rin = (key % a.cells) / (uint32_t)a.ncx;      // cz * ncy + cy
    const int cy = (int)(rin % (uint32_t)a.ncy), cz = (int)(rin / (uint32_t)a.ncy);
    const int64_t slot0 = (MODE == GS_WRITE && in) ? a.rowptr[i] : 0;
    int cnt = 0;

    uint64_t todo = __ballot(live);
    while (todo) {
        // the next row piece: the sorted lanes of one x-row are adjacent and ascend in cx
        const int first = __ffsll((unsigned long long)todo) - 1;
        const uint32_t R = (uint32_t)__builtin_amdgcn_readlane((int)rowkey, first);
        const bool mine = live && rowkey == R;
        const uint64_t m = __ballot(mine);
        todo &= ~m;
        const int last = 63 - __clzll((unsigned long long)m);
        const int xa = max(__builtin_amdgcn_readlane(cx, first) - 1, 0);
        const int xb = min(__builtin_amdgcn_readlane(cx, last) + 1, a.ncx - 1);
        const int ry = __builtin_amdgcn_readlane(cy, first), rz = __builtin_amdgcn_readlane(cz, first);
        for (int dz = -1; dz <= 1; ++dz) {
            if (rz + dz < 0 || rz + dz >= a.ncz) continue;
            for (int dy = -1; dy <= 1; ++dy) {
                if (ry + dy < 0 || ry + dy >= a.ncy) continue;
                // (the neighbour row is in the same graph: only cz and cy moved, inside their ranges)
                const uint32_t rk = (uint32_t)((int64_t)R + dz * a.ncy + dy) * (uint32_t)a.ncx;
                const uint32_t q0 = a.start[rk + (uint32_t)xa], q1 = a.start[rk + (uint32_t)xb + 1u];
                float4 nxt = (q0 + lane < q1) ? a.rec[q0 + lane] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                for (uint32_t q = q0; q < q1; q += GS_TILE) {
                    __syncthreads();                 // the readers of the tile before are done
                    tile[lane] = nxt;
                    __syncthreads();
                    const uint32_t qn = q + GS_TILE + lane;
                    if (qn < q1) nxt = a.rec[qn];
                    const int n = (int)min((uint32_t)GS_TILE, q1 - q);
#pragma unroll 4
                    for (int t = 0; t < n; ++t) {
                        const float4 v = tile[t];
                        const float dx = me.x - v.x, dyy = me.y - v.y, dzz = me.z - v.z;
                        float acc = __builtin_fmaf(dx, dx, 0.0f);
                        acc = __builtin_fmaf(dyy, dyy, acc);
                        acc = __builtin_fmaf(dzz, dzz, acc);
                        const uint32_t j = __float_as_uint(v.w);
                        // (r2 is finite on this route: a NaN or infinite d2 is no hit, which is "ranks as +inf")
                        const bool hit = mine && acc <= a.r2 && (a.self_loops || j != i);
                        if (MODE == GS_WRITE && hit) {
                            const int64_t e = slot0 + cnt;
                            a.col[e] = (int32_t)j;
                            a.eid[e] = (int32_t)(uint32_t)e;
                        }
                        cnt += hit ? 1 : 0;
                    }
                }
            }
        }
    }
    if (MODE == GS_COUNT) {
        if (in) a.deg[i] = cnt;
        int mx = cnt;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) mx = max(mx, __shfl_xor(mx, o, 64));
        if (lane == 0 && mx > 0) atomicMax(a.max_deg, (unsigned long long)mx);
    }
}

// one group of LG lanes a row of at most CAP entries: ranks through LDS
template <int LG, int CAP>
__global__ void __launch_bounds__(256) grid_row_order_kernel(const int64_t *rowptr, int32_t *col, int64_t N) {
    __shared__ int32_t buf[(256 / LG) * CAP];
    const int grp = threadIdx.x / LG, l = threadIdx.x % LG;
    const int64_t row = (int64_t)blockIdx.x * (256 / LG) + grp;
    int64_t b = 0;
    int n = 0;
    if (row < N) {
        b = rowptr[row];
        n = (int)min((int64_t)CAP, rowptr[row + 1] - b);   // (the host checked the largest degree against CAP)
    }
    int32_t *mine = buf + grp * CAP;
    for (int t = l; t < n; t += LG) mine[t] = col[b + t];
    __syncthreads();
    for (int t = l; t < n; t += LG) {
        const int32_t v = mine[t];
        int rank = 0;
        for (int s = 0; s < n; ++s) rank += mine[s] < v ? 1 : 0;
        col[b + rank] = v;
    }
}

inline unsigned gblk(int64_t n, int bs = 256) { return (unsigned)((n + bs - 1) / bs); }

GridSearchArgs search_args(const GridIndex &ix, float r2, int self_loops) {
    GridSearchArgs a{};
    a.keys = ix.keys.get();
    a.start = ix.start.get();
    a.rec = ix.rec.get();
    a.N = ix.N;
    a.ncx = ix.geo.nc[0];
    a.ncy = ix.geo.nc[1];
    a.ncz = ix.geo.nc[2];
    a.cells = (uint32_t)ix.geo.cells;
    a.none = (uint32_t)(ix.geo.table - 1);
    a.r2 = r2;
    a.self_loops = self_loops ? 1 : 0;
    return a;
}

}  // namespace

int grid_bbox(const float *x, int64_t N, int d, hipStream_t stream, NbBox &box) {
    DevBuf<GridStats> st;
    GridStats h;
    GNNMP_HIP(st.alloc(1));
    grid_stats_init_kernel<<<1, 64, 0, stream>>>(st.get());
    GNNMP_LAUNCH_CHECK("grid_stats_init_kernel");
    grid_bbox_kernel<<<std::min<unsigned>(gblk(N), (unsigned)device_cus() * 8u), 256, 0, stream>>>(x, N, d, st.get());
    GNNMP_LAUNCH_CHECK("grid_bbox_kernel");
    GNNMP_HIP(hipMemcpyAsync(&h, st.get(), sizeof(h), hipMemcpyDeviceToHost, stream));
    GNNMP_HIP(hipStreamSynchronize(stream));
    box.n_finite = (int64_t)h.n_finite;
    for (int c = 0; c < 3; ++c) {
        const bool have = c < d && h.n_finite > 0;
        box.lo[c] = have ? (double)ord_dec(h.lo[c]) : 0.0;
        box.hi[c] = have ? (double)ord_dec(h.hi[c]) : 0.0;
    }
    return GNNMP_OK;
}

int grid_build(GridIndex &ix, const NbGrid &geo, const float *x, int64_t N, int d, const void *gi, int gi_bytes, int base,
               hipStream_t stream) {
    ix.geo = geo;
    ix.N = N;
    GridGeoDev g;
    for (int c = 0; c < 3; ++c) {
        g.o[c] = geo.origin[c];
        g.nc[c] = geo.nc[c];
    }
    g.h = geo.h;
    g.cells = (uint32_t)geo.cells;
    g.none = (uint32_t)(geo.table - 1);
    DevBuf<uint32_t> keys0, vals0, order;
    GNNMP_HIP(keys0.alloc((size_t)N));
    GNNMP_HIP(vals0.alloc((size_t)N));
    GNNMP_HIP(order.alloc((size_t)N));
    GNNMP_HIP(ix.keys.alloc((size_t)N));
    GNNMP_HIP(ix.start.alloc((size_t)geo.table));
    GNNMP_HIP(ix.rec.alloc((size_t)N));
    grid_key_kernel<<<gblk(N), 256, 0, stream>>>(x, N, d, gi, gi_bytes, base, g, keys0.get(), vals0.get());
    GNNMP_LAUNCH_CHECK("grid_key_kernel");
    int bits = 1;
    while (bits < 32 && ((uint64_t)g.none >> bits) != 0) ++bits;
    // (LSD radix passes are stable: equal keys keep the ascending j they start with)
    GNNMP_TRY(radix_sort_pairs_u32(keys0.get(), ix.keys.get(), vals0.get(), order.get(), (size_t)N, 0, bits, stream));
    grid_cell_start_kernel<<<gblk(geo.table), 256, 0, stream>>>(ix.keys.get(), N, geo.table, ix.start.get());
    GNNMP_LAUNCH_CHECK("grid_cell_start_kernel");
    grid_pack_kernel<<<gblk(N), 256, 0, stream>>>(x, N, d, order.get(), ix.rec.get());
    GNNMP_LAUNCH_CHECK("grid_pack_kernel");
    return GNNMP_OK;   // (keys0, vals0, order: hipFree waits for the kernels that read them)
}

int grid_count(const GridIndex &ix, float r2, int self_loops, int64_t *deg, int64_t *max_deg, hipStream_t stream) {
    GridSearchArgs a = search_args(ix, r2, self_loops);
    a.deg = deg;
    a.max_deg = reinterpret_cast<unsigned long long *>(max_deg);
    grid_search_kernel<GS_COUNT><<<gblk(ix.N, GS_TILE), GS_TILE, 0, stream>>>(a);
    GNNMP_LAUNCH_CHECK("grid_search_kernel<count>");
    return GNNMP_OK;
}

int grid_write(const GridIndex &ix, float r2, int self_loops, const int64_t *rowptr, int32_t *col, int32_t *eid, int64_t max_deg,
               hipStream_t stream) {
    if (max_deg > NB_GRID_ROW_CAP) return fail(GNNMP_EINVAL, "grid_write: a row of %lld entries", (long long)max_deg);
    GridSearchArgs a = search_args(ix, r2, self_loops);
    a.rowptr = rowptr;
    a.col = col;
    a.eid = eid;
    grid_search_kernel<GS_WRITE><<<gblk(ix.N, GS_TILE), GS_TILE, 0, stream>>>(a);
    GNNMP_LAUNCH_CHECK("grid_search_kernel<write>");
    if (max_deg <= 1) return GNNMP_OK;
    if (max_deg <= 64)
        grid_row_order_kernel<16, 64><<<gblk(ix.N, 16), 256, 0, stream>>>(rowptr, col, ix.N);
    else
        grid_row_order_kernel<64, NB_GRID_ROW_CAP><<<gblk(ix.N, 4), 256, 0, stream>>>(rowptr, col, ix.N);
    GNNMP_LAUNCH_CHECK("grid_row_order_kernel");
    return GNNMP_OK;
}

}  // namespace gnnmp
