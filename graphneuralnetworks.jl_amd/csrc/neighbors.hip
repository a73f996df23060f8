// neighbors.hip — exact neighbour search on the device: the graph constructors
//   knn_graph(points, k; graph_indicator, self_loops, dir)      GNNGraphs/src/generate.jl:112-145
//   radius_graph(points, r; graph_indicator, self_loops, dir)   GNNGraphs/src/generate.jl:196-222
//   hyperbolic_graph(points, R, zeta; ...)                      the N x N loop of rand_temporal_hyperbolic_graph, generate.jl:287-297, 359-369
// The reference builds a KDTree / BallTree on the CPU (NearestNeighbors.jl).  Here: brute force in fp32, one kernel skeleton for both.
//
// Semantics (gnnmp.h states them for callers): d2(i, j) = fma chain over the dimensions in order, a non-finite d2 ranks as +inf,
// candidates are ordered by the pair (d2, j) — a total order, so the result does not depend on the tiling and reruns are bit-identical.
//
// Shape.  A block of 4 waves owns 16 consecutive queries, 4 per wave.  The candidates of the block (the segment(s) of its queries, or
// everything) are staged through LDS in tiles of 64 rows x 32 dimensions (row stride 33 floats: lane l reads row l, conflict free); the
// 4 queries of a wave are read from LDS as one float4 broadcast per dimension, so a dimension costs a lane 2 LDS reads and 8 VALU ops
// for 4 pairs.  Every lane then holds the distance of ITS candidate to each of the wave's 4 queries.
// The best-k list of a query is held ACROSS the wave — lane r holds the r-th best (key = d2 bits << 32 | j, a plain unsigned compare) —
// not in a per-lane register array: there is nothing to index at run time (no scratch at any k), and an insertion is one wave-uniform
// step (shift the tail by one lane with a DPP move, drop the candidate into the gap) instead of a divergent pass that a wave of 64
// independent per-lane lists pays 64 times over.  A tile's candidates below the current k-th key are found with one ballot and inserted
// one by one; after the first tiles almost every tile is rejected by the ballot alone.  k > 64: ceil(k / 64) passes, each keeping the
// best 64 keys strictly above the last key of the pass before.
// radius_graph: the same distances; a count pass (ballot + popcount), an exclusive scan, and a write pass whose position inside a row
// is the popcount of the lanes below — neighbours ascend in j by construction.  No atomics in any of the search kernels.
// hyperbolic_graph: the radius skeleton with another pair value.  The reference's rule acosh(cosh a_i cosh a_j - sinh a_i sinh a_j cos(dtheta))
// <= zeta R (a = zeta r) is, acosh being monotone, 2 v <= 2 cosh(zeta R) with
//     2 v = (E_i F_j + F_i E_j) + S_i S_j h,   E = e^a, F = e^-a, S = sinh a, h = 4 sin^2(dtheta / 2) = (c_i - c_j)^2 + (s_i - s_j)^2,
// two non-negative terms: nothing cancels.  A pre-pass computes per NODE, in double, E, F, S (rounded to fp32 once) and c = cos theta,
// s = sin theta (kept in double: a float32 difference of two angles on either side of the 0 / 2 pi seam has lost the digits that matter;
// the chord of two unit vectors has not) into scoped scratch, 32 bytes a node; a PAIR is then two double subtractions, a double
// multiply and multiply-add, one conversion and five fp32 operations — no transcendental.  A lane reads its candidate's record and the wave's four
// query records straight from that array (one record is everything a pair needs: there is no tile to transpose through LDS).
// Output.  Edge e = (centre i, its r-th neighbour) of the reference's adjacency list -> COO conversion is destination-sorted as produced,
// so the kernels write the graph's PLAN directly (row i = centre i, col = neighbour, eid[e] = e): what gnnmp_plan_from_csc would build
// from (colptr, rowval), without the copy.  (s, t) in any index width and base come from gnnmp_plan_edge_index.
#include <algorithm>
#include <cmath>

#include "common.h"
#include "scratch.h"
#include "sort_scan.h"

namespace gnnmp {
namespace {

constexpr int NB_WAVES = 4;             // waves per block
constexpr int NB_QW = 4;                // queries per wave (one float4 of query coordinates per dimension)
constexpr int NB_QB = NB_WAVES * NB_QW; // queries per block
constexpr int NB_TILE = 64;             // candidates per tile: one per lane
constexpr int NB_DCH = 32;              // dimensions per LDS chunk
constexpr int NB_LD = NB_DCH + 1;       // row stride of the candidate tile (odd: lane l -> bank (l + c) % 32)
constexpr uint64_t NB_NONE = ~0ULL;     // "no candidate": above every real key (d2 bits <= 0x7f800000)
constexpr int NB_MAX_K = 1024;

enum { NB_KNN = 0, NB_COUNT = 1, NB_WRITE = 2 };
enum { NB_L2 = 0, NB_HYP = 1 };         // the pair value: squared Euclidean distance | 2 cosh(zeta d_hyperbolic)

// what a pair needs of a node of the hyperbolic plane (r, theta): c, s = cos, sin theta in double; E, F, S = e^(zeta r), e^(-zeta r),
// sinh(zeta r) computed in double and rounded to fp32 once; ok = 0 when r or theta is not finite
struct HypNode {
    double c, s;
    float E, F, S;
    int ok;
};
static_assert(sizeof(HypNode) == 32, "one node is 32 bytes");

struct NbArgs {
    const float *x;           // [N][d]
    int64_t N;
    int d;
    const int64_t *seg_ptr;   // sorted indicator: first node of every graph, [G + 1]; else nullptr
    const void *gi;           // graph id of every node (nullptr: one graph)
    int gi_bytes, base;
    int self_loops;
    int k;                    // knn
    float r2;                 // radius
    const int64_t *rowptr;    // radius, write pass: first edge of every centre
    int64_t *deg;             // radius, count pass
    int32_t *col, *eid;       // the plan's slots: slot e = edge e (row = centre, col = neighbour)
    const HypNode *hyp;       // hyperbolic: the per-node records [N] (x is not read by the search then)
};

// lane r <- lane r - 1 over the whole wave (DPP wave_shr:1; lane 0 keeps its own value, the caller ignores it)
__device__ __forceinline__ uint32_t lane_shr1(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x138, 0xf, 0xf, false);
}
__device__ __forceinline__ uint64_t lane_shr1_64(uint64_t v) {
    return ((uint64_t)lane_shr1((uint32_t)(v >> 32)) << 32) | lane_shr1((uint32_t)v);
}
__device__ __forceinline__ uint64_t readlane_64(uint64_t v, int lane) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, lane);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), lane);
    return ((uint64_t)hi << 32) | lo;
}

// edge e of the adjacency list -> COO conversion (convert.jl:97-117) is slot e of the plan: row = centre, source = neighbour
__device__ __forceinline__ void store_edge(const NbArgs &a, int64_t e, int64_t nb) {
    a.col[e] = (int32_t)nb;
    a.eid[e] = (int32_t)(uint32_t)e;
}

// the hyperbolic pre-pass: one record a node.  zeta * r is exact in double (two fp32 factors); exp / sinh / sincos in double are
// within 2 ulp of double, so E, F, S carry the one fp32 rounding and c, s about 2^-52.
__global__ void hyp_nodes_kernel(const float *points, int64_t N, double zeta, HypNode *out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const float r = points[2 * i], th = points[2 * i + 1];
    const double ar = zeta * (double)r;
    HypNode n;
    sincos((double)th, &n.s, &n.c);
    n.E = (float)exp(ar);
    n.F = (float)exp(-ar);
    n.S = (float)sinh(ar);
    n.ok = (r - r == 0.0f && th - th == 0.0f) ? 1 : 0;
    out[i] = n;
}

// 2 v(q, c) for two DISTINCT nodes (see the head of the file); equal radii (E equal in fp32: cosh(zeta dr) - 1 < 2^-46) give the
// first term as the exact 2, so that coincident points have v = 1 <= cosh(zeta R) at every R >= 0
__device__ __forceinline__ float hyp_pair(const HypNode &q, const HypNode &c) {
    const double dc = q.c - c.c, ds = q.s - c.s;
    const float h = (float)__builtin_fma(ds, ds, dc * dc);
    const float t = q.E == c.E ? 2.0f : __builtin_fmaf(q.F, c.E, q.E * c.F);
    return t + (q.S * c.S) * h;
}

template <int MODE, int METRIC = NB_L2>
__global__ void __launch_bounds__(256) neighbors_kernel(const NbArgs a) {
    __shared__ float cand[NB_TILE * NB_LD];
    __shared__ float4 qs[NB_WAVES][NB_DCH];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int d = a.d;
    const int64_t qb0 = (int64_t)blockIdx.x * NB_QB;           // (the grid covers N: qb0 < N)
    const int64_t qb1 = min(qb0 + NB_QB, a.N);
    // the block's candidate range: from the first query's segment to the last one's
    int64_t blo = 0, bhi = a.N;
    if (a.seg_ptr) {
        blo = a.seg_ptr[load_index(a.gi, qb0, a.gi_bytes, a.base)];
        bhi = a.seg_ptr[load_index(a.gi, qb1 - 1, a.gi_bytes, a.base) + 1];
    }
    int64_t qi[NB_QW], lo[NB_QW], hi[NB_QW], qg[NB_QW];
    bool live[NB_QW];
#pragma unroll
    for (int q = 0; q < NB_QW; ++q) {
        qi[q] = qb0 + wave * NB_QW + q;
        live[q] = qi[q] < a.N;
        lo[q] = 0;
        hi[q] = a.N;
        qg[q] = 0;
        if (live[q] && a.gi) {
            qg[q] = load_index(a.gi, qi[q], a.gi_bytes, a.base);
            if (a.seg_ptr) {
                lo[q] = a.seg_ptr[qg[q]];
                hi[q] = a.seg_ptr[qg[q] + 1];
            }
        }
    }
    HypNode hq[NB_QW];                          // hyperbolic: the wave's queries (wave-uniform)
    if (METRIC == NB_HYP) {
#pragma unroll
        for (int q = 0; q < NB_QW; ++q) hq[q] = a.hyp[live[q] ? qi[q] : qb0];
    }
    const bool mask_ids = a.gi && !a.seg_ptr;   // unsorted indicator: full range, other graphs masked
    const int n_pass = MODE == NB_KNN ? (a.k + 63) / 64 : 1;
    const bool one_chunk = d <= NB_DCH;
    uint64_t lb[NB_QW];                         // last key of the pass before (exclusive lower bound)
#pragma unroll
    for (int q = 0; q < NB_QW; ++q) lb[q] = 0;

    for (int pass = 0; pass < n_pass; ++pass) {
        const int kk = MODE == NB_KNN ? min(64, a.k - 64 * pass) : 0;
        uint64_t best[NB_QW], thr[NB_QW];       // best: lane r holds the r-th smallest key so far; thr: the kk-th (wave-uniform)
        int64_t cnt[NB_QW];
#pragma unroll
        for (int q = 0; q < NB_QW; ++q) {
            best[q] = NB_NONE;
            thr[q] = NB_NONE;
            cnt[q] = 0;
        }
        for (int64_t tile0 = blo; tile0 < bhi; tile0 += NB_TILE) {
            float acc[NB_QW];
#pragma unroll
            for (int q = 0; q < NB_QW; ++q) acc[q] = 0.0f;
            if (METRIC == NB_HYP) {
                const int64_t jc = tile0 + lane;
                const HypNode cn = a.hyp[jc < bhi ? jc : blo];      // (past the range: any record, the lane is masked below)
#pragma unroll
                for (int q = 0; q < NB_QW; ++q) {
                    const bool fin = hq[q].ok && cn.ok;
                    acc[q] = !fin ? __builtin_nanf("") : (jc == qi[q] ? 2.0f : hyp_pair(hq[q], cn));   // (a node to itself: v = 1)
                }
            }
            for (int ch0 = 0; METRIC == NB_L2 && ch0 < d; ch0 += NB_DCH) {
                const int cw = min(NB_DCH, d - ch0);
                __syncthreads();                // the readers of the chunk before are done
                for (int idx = tid; idx < NB_TILE * cw; idx += 256) {
                    const int row = idx / cw, c = idx - row * cw;
                    const int64_t j = tile0 + row;
                    cand[row * NB_LD + c] = j < bhi ? a.x[j * d + ch0 + c] : 0.0f;
                }
                if (!one_chunk || (pass == 0 && tile0 == blo)) {   // (one chunk: the queries stay in LDS for the whole kernel)
                    for (int idx = tid; idx < NB_QB * cw; idx += 256) {
                        const int qq = idx / cw, c = idx - qq * cw;
                        const int64_t qn = qb0 + qq;
                        reinterpret_cast<float *>(&qs[qq / NB_QW][c])[qq % NB_QW] = qn < a.N ? a.x[qn * d + ch0 + c] : 0.0f;
                    }
                }
                __syncthreads();
                for (int c = 0; c < cw; ++c) {
                    const float v = cand[lane * NB_LD + c];
                    const float4 xq = qs[wave][c];
                    const float d0 = xq.x - v, d1 = xq.y - v, d2 = xq.z - v, d3 = xq.w - v;
                    acc[0] = __builtin_fmaf(d0, d0, acc[0]);
                    acc[1] = __builtin_fmaf(d1, d1, acc[1]);
                    acc[2] = __builtin_fmaf(d2, d2, acc[2]);
                    acc[3] = __builtin_fmaf(d3, d3, acc[3]);
                }
            }
            const int64_t j = tile0 + lane;
            int64_t jg = 0;
            if (mask_ids && j < a.N) jg = load_index(a.gi, j, a.gi_bytes, a.base);
#pragma unroll
            for (int q = 0; q < NB_QW; ++q) {
                if (!live[q]) continue;         // (wave-uniform)
                bool ok = j >= lo[q] && j < hi[q] && (a.self_loops || j != qi[q]);
                if (mask_ids) ok = ok && jg == qg[q];
                float dd = acc[q];
                if (!(dd < __builtin_inff())) dd = __builtin_inff();   // NaN and +inf rank last
                if (MODE == NB_KNN) {
                    uint64_t key = ok ? (((uint64_t)__float_as_uint(dd) << 32) | (uint64_t)(uint32_t)j) : NB_NONE;
                    if (pass > 0 && key <= lb[q]) key = NB_NONE;
                    uint64_t m = __ballot(key < thr[q]);
                    while (m) {
                        const int b = __ffsll((unsigned long long)m) - 1;
                        m &= m - 1;
                        const uint64_t ck = readlane_64(key, b);
                        if (ck < thr[q]) {      // (the threshold may have dropped since the ballot)
                            const uint64_t up = lane_shr1_64(best[q]);
                            const bool gt = best[q] > ck;
                            const bool up_gt = lane > 0 && up > ck;
                            best[q] = gt ? (up_gt ? up : ck) : best[q];
                            thr[q] = readlane_64(best[q], kk - 1);
                        }
                    }
                } else {
                    // (hyperbolic: a value that is not finite is no edge even when cosh(zeta R) itself overflowed to +inf)
                    const uint64_t m = __ballot(ok && dd <= a.r2 && (METRIC == NB_L2 || dd < __builtin_inff()));
                    if (MODE == NB_WRITE) {
                        if ((m >> lane) & 1ULL) {
                            const int64_t e = a.rowptr[qi[q]] + cnt[q] + __popcll(m & ((1ULL << lane) - 1ULL));
                            store_edge(a, e, j);
                        }
                    }
                    cnt[q] += __popcll(m);
                }
            }
        }
#pragma unroll
        for (int q = 0; q < NB_QW; ++q) {
            if (!live[q]) continue;
            if (MODE == NB_KNN) {
                // (every graph holds at least k candidates, checked before the launch: the first kk lanes hold real keys)
                if (lane < kk) store_edge(a, qi[q] * a.k + 64 * pass + lane, (int64_t)(uint32_t)best[q]);
                lb[q] = readlane_64(best[q], 63);
            } else if (MODE == NB_COUNT) {
                if (lane == 0) a.deg[qi[q]] = cnt[q];
            }
        }
    }
}

// flags[0] |= 1: the indicator decreases somewhere; flags[1] |= 1: an id outside 0..G-1
__global__ void gi_check_kernel(const void *gi, int gi_bytes, int base, int64_t N, int64_t G, int *flags) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const int64_t g = load_index(gi, i, gi_bytes, base);
    if (g < 0 || g >= G) flags[1] = 1;
    if (i > 0 && load_index(gi, i - 1, gi_bytes, base) > g) flags[0] = 1;
}
// graph sizes of an UNSORTED indicator (integer adds: the counts do not depend on the order)
__global__ void gi_hist_kernel(const void *gi, int gi_bytes, int base, int64_t N, unsigned long long *counts) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    atomicAdd(&counts[load_index(gi, i, gi_bytes, base)], 1ULL);
}
// flags[2] |= 1: a graph that has nodes has fewer than `need` (countmap holds only the ids that occur, generate.jl:122-123)
__global__ void seg_min_kernel(const int64_t *v, int diff, int64_t G, int64_t need, int *flags) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= G) return;
    const int64_t c = diff ? v[g + 1] - v[g] : v[g];
    if (c > 0 && c < need) flags[2] = 1;
}

inline unsigned nblk(int64_t n, int bs = 256) { return (unsigned)((n + bs - 1) / bs); }

// The indicator's checks and, when it is non-decreasing, its segment boundaries (seg: left empty when unsorted).
// `need` > 0: every graph that occurs must hold at least `need` nodes.  Synchronises the stream (once; twice when unsorted).
int prepare_indicator(const char *who, const void *gi, int gi_bytes, int base, int64_t N, int64_t G, int64_t need, hipStream_t stream,
                      DevBuf<int64_t> &seg) {
    DevBuf<int> flags;
    DevBuf<int64_t> sp;
    int h[4] = {0, 0, 0, 0};
    GNNMP_HIP(sp.alloc((size_t)(G + 1)));
    GNNMP_HIP(flags.alloc(4));
    GNNMP_HIP(hipMemsetAsync(flags.get(), 0, sizeof(int) * 4, stream));
    gi_check_kernel<<<nblk(N), 256, 0, stream>>>(gi, gi_bytes, base, N, G, flags.get());
    GNNMP_HIP(hipGetLastError());
    GNNMP_TRY(gnnmp_segment_bounds(gi, gi_bytes, base, N, G, sp.get(), (gnnmp_stream_t)stream));   // (stays inside [0, G] on any input)
    if (need > 0) {
        seg_min_kernel<<<nblk(G), 256, 0, stream>>>(sp.get(), 1, G, need, flags.get());
        GNNMP_HIP(hipGetLastError());
    }
    GNNMP_HIP(hipMemcpyAsync(h, flags.get(), sizeof(int) * 4, hipMemcpyDeviceToHost, stream));
    GNNMP_HIP(hipStreamSynchronize(stream));
    if (h[1]) return fail(GNNMP_EBOUNDS, "%s: a graph_indicator entry is outside the %lld graphs", who, (long long)G);
    if (h[0] && need > 0) {   // unsorted: the boundaries mean nothing, count the ids
        GNNMP_HIP(hipMemsetAsync(sp.get(), 0, sizeof(int64_t) * (size_t)(G + 1), stream));
        GNNMP_HIP(hipMemsetAsync(flags.get(), 0, sizeof(int) * 4, stream));
        gi_hist_kernel<<<nblk(N), 256, 0, stream>>>(gi, gi_bytes, base, N, reinterpret_cast<unsigned long long *>(sp.get()));
        GNNMP_HIP(hipGetLastError());
        seg_min_kernel<<<nblk(G), 256, 0, stream>>>(sp.get(), 0, G, need, flags.get());
        GNNMP_HIP(hipGetLastError());
        GNNMP_HIP(hipMemcpyAsync(h + 2, flags.get() + 2, sizeof(int), hipMemcpyDeviceToHost, stream));
        GNNMP_HIP(hipStreamSynchronize(stream));
    }
    if (need > 0 && h[2]) return fail(GNNMP_EBOUNDS, "%s: a graph of the batch has fewer than %lld nodes", who, (long long)need);
    if (!h[0]) seg = std::move(sp);
    return GNNMP_OK;
}

// rowptr[i] = i k (knn: every row holds k slots)
__global__ void knn_rowptr_kernel(uint32_t *rowptr, int64_t N, int64_t k) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i <= N) rowptr[i] = (uint32_t)(i * k);
}
__global__ void narrow_rowptr_kernel(const int64_t *in, uint32_t *rowptr, int64_t N) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i <= N) rowptr[i] = (uint32_t)in[i];
}

// argument checks shared by the two entry points; no HIP call
int check_common(const char *who, gnnmp_graph_t **out, const float *points, int64_t N, int64_t d, const void *gi, int gi_bytes,
                 int index_base, int64_t G) {
    if (!out) return fail(GNNMP_EINVAL, "%s: out is NULL", who);
    *out = nullptr;
    if (N < 0) return fail(GNNMP_EINVAL, "%s: N = %lld < 0", who, (long long)N);
    if (d < 1) return fail(GNNMP_EINVAL, "%s: d = %lld < 1", who, (long long)d);
    if (gi && gi_bytes != 4 && gi_bytes != 8) return fail(GNNMP_EINVAL, "%s: idx_bytes %d", who, gi_bytes);
    if (gi && index_base != 0 && index_base != 1) return fail(GNNMP_EINVAL, "%s: index_base %d", who, index_base);
    if (gi && G < 1) return fail(GNNMP_EINVAL, "%s: n_graphs = %lld < 1", who, (long long)G);
    if (N > 0 && !points) return fail(GNNMP_EINVAL, "%s: null points", who);
    if (N >= (int64_t)INT32_MAX || d > (1 << 20)) return fail(GNNMP_EUNSUPPORTED, "%s: N >= 2^31 - 1 or d > 2^20", who);
    return GNNMP_OK;
}

NbArgs make_args(const float *points, int64_t N, int64_t d, const void *gi, int gi_bytes, int index_base, const int64_t *seg_ptr,
                 int self_loops, const gnnmp_graph_t *p) {
    NbArgs a;
    a.x = points;
    a.N = N;
    a.d = (int)d;
    a.seg_ptr = seg_ptr;
    a.gi = gi;
    a.gi_bytes = gi_bytes;
    a.base = index_base;
    a.self_loops = self_loops ? 1 : 0;
    a.k = 0;
    a.r2 = 0.0f;
    a.rowptr = nullptr;
    a.deg = nullptr;
    a.col = p->col;
    a.eid = p->eid;
    a.hyp = nullptr;
    return a;
}

// the plan's arrays for n_dst = n_src = N rows and E slots (what gnnmp_plan_from_csc allocates)
int alloc_plan_rows(gnnmp_graph_t *p, int64_t N) {
    p->n_src = p->n_dst = N;
    GNNMP_HIP(alloc_into(p->rowptr, (size_t)(N + 1)));
    return GNNMP_OK;
}
int alloc_plan_slots(gnnmp_graph_t *p, int64_t E) {
    const size_t epad = (size_t)std::max<int64_t>(E, 1);
    p->n_edges = p->n_total = E;
    p->long_thresh = plan_long_thresh(E);
    GNNMP_HIP(alloc_into(p->col, epad));
    GNNMP_HIP(alloc_into(p->eid, epad));
    p->bytes = (int64_t)(sizeof(int32_t) * ((size_t)(p->n_dst + 1) + 2 * epad));
    return GNNMP_OK;
}

// Every pair whose value is at most `thr`, as a plan: the count pass, the scan (its total is read on the host: it sizes the plan) and the
// write pass, for either pair value.  The arguments have been checked.  hyp: the per-node records of the hyperbolic value (else nullptr).
template <int METRIC>
int threshold_graph(const char *who, gnnmp_graph_t **out, const float *points, int64_t N, int64_t d, float thr, const HypNode *hyp,
                    const void *graph_indicator, int idx_bytes, int index_base, int64_t n_graphs, int self_loops, hipStream_t stream) {
    PlanPtr p(new gnnmp_graph_t());
    // (rowptr64 dies when the call returns: after plan_build_long_rows' synchronisation, or its hipFree waits itself)
    DevBuf<int64_t> rowptr64, seg;
    if (graph_indicator && N > 0)
        GNNMP_TRY(prepare_indicator(who, graph_indicator, idx_bytes, index_base, N, n_graphs, 0, stream, seg));
    GNNMP_TRY(alloc_plan_rows(p.get(), N));
    GNNMP_HIP(rowptr64.alloc((size_t)(N + 1)));
    NbArgs a = make_args(points, N, d, graph_indicator, idx_bytes, index_base, seg.get(), self_loops, p.get());
    a.r2 = thr;
    a.hyp = hyp;
    GNNMP_HIP(hipMemsetAsync(rowptr64.get() + N, 0, sizeof(int64_t), stream));
    if (N > 0) {
        a.deg = rowptr64.get();
        neighbors_kernel<NB_COUNT, METRIC><<<nblk(N, NB_QB), 256, 0, stream>>>(a);
        GNNMP_HIP(hipGetLastError());
    }
    GNNMP_TRY(exclusive_scan_i64(rowptr64.get(), rowptr64.get(), (size_t)(N + 1), stream));
    int64_t tot = 0;
    GNNMP_HIP(hipMemcpyAsync(&tot, rowptr64.get() + N, sizeof(int64_t), hipMemcpyDeviceToHost, stream));
    GNNMP_HIP(hipStreamSynchronize(stream));
    if (tot >= (int64_t)GNNMP_MAX_SLOTS) return fail(GNNMP_EUNSUPPORTED, "%s: %lld edges exceed the plan format", who, (long long)tot);
    GNNMP_TRY(alloc_plan_slots(p.get(), tot));
    narrow_rowptr_kernel<<<nblk(N + 1), 256, 0, stream>>>(rowptr64.get(), p->rowptr, N);
    GNNMP_HIP(hipGetLastError());
    if (tot > 0) {
        a.col = p->col;
        a.eid = p->eid;
        a.rowptr = rowptr64.get();
        neighbors_kernel<NB_WRITE, METRIC><<<nblk(N, NB_QB), 256, 0, stream>>>(a);
        GNNMP_HIP(hipGetLastError());
    }
    GNNMP_TRY(plan_build_long_rows(p.get(), stream));
    *out = p.release();
    return GNNMP_OK;
}

}  // namespace
}  // namespace gnnmp

using namespace gnnmp;

extern "C" {

int gnnmp_knn_graph_f32(gnnmp_graph_t **out, const float *points, int64_t N, int64_t d, int64_t k, const void *graph_indicator,
                        int idx_bytes, int index_base, int64_t n_graphs, int self_loops, gnnmp_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    GNNMP_TRY(check_common("knn_graph", out, points, N, d, graph_indicator, idx_bytes, index_base, n_graphs));
    if (k < 1) return fail(GNNMP_EINVAL, "knn_graph: k = %lld < 1", (long long)k);
    if (k > NB_MAX_K) return fail(GNNMP_EINVAL, "knn_graph: k = %lld > %d", (long long)k, NB_MAX_K);
    if (N * k >= (int64_t)GNNMP_MAX_SLOTS) return fail(GNNMP_EUNSUPPORTED, "knn_graph: N k exceeds the plan format");
    const int64_t need = k + (self_loops ? 0 : 1);
    if (N > 0 && N < need) return fail(GNNMP_EBOUNDS, "knn_graph: %lld points, fewer than %lld", (long long)N, (long long)need);
    PlanPtr p(new gnnmp_graph_t());
    DevBuf<int64_t> seg;
    if (graph_indicator && N > 0)
        GNNMP_TRY(prepare_indicator("knn_graph", graph_indicator, idx_bytes, index_base, N, n_graphs, need, stream, seg));
    GNNMP_TRY(alloc_plan_rows(p.get(), N));
    GNNMP_TRY(alloc_plan_slots(p.get(), N * k));
    knn_rowptr_kernel<<<nblk(N + 1), 256, 0, stream>>>(p->rowptr, N, k);
    GNNMP_HIP(hipGetLastError());
    if (N > 0) {
        NbArgs a = make_args(points, N, d, graph_indicator, idx_bytes, index_base, seg.get(), self_loops, p.get());
        a.k = (int)k;
        neighbors_kernel<NB_KNN><<<nblk(N, NB_QB), 256, 0, stream>>>(a);
        GNNMP_HIP(hipGetLastError());
    }
    GNNMP_TRY(plan_build_long_rows(p.get(), stream));   // (synchronises the stream, as every plan build does)
    *out = p.release();
    return GNNMP_OK;
}

int gnnmp_radius_graph_f32(gnnmp_graph_t **out, const float *points, int64_t N, int64_t d, float r, const void *graph_indicator,
                           int idx_bytes, int index_base, int64_t n_graphs, int self_loops, gnnmp_stream_t stream_) {
    GNNMP_TRY(check_common("radius_graph", out, points, N, d, graph_indicator, idx_bytes, index_base, n_graphs));
    if (!(r >= 0.0f)) return fail(GNNMP_EINVAL, "radius_graph: r = %g (negative or NaN)", (double)r);
    return threshold_graph<NB_L2>("radius_graph", out, points, N, d, r * r, nullptr, graph_indicator, idx_bytes, index_base, n_graphs,
                                  self_loops, (hipStream_t)stream_);
}

int gnnmp_hyperbolic_graph_f32(gnnmp_graph_t **out, const float *points, int64_t N, float R, float zeta, const void *graph_indicator,
                               int idx_bytes, int index_base, int64_t n_graphs, int self_loops, gnnmp_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    GNNMP_TRY(check_common("hyperbolic_graph", out, points, N, 2, graph_indicator, idx_bytes, index_base, n_graphs));
    if (!(R >= 0.0f)) return fail(GNNMP_EINVAL, "hyperbolic_graph: R = %g (negative or NaN)", (double)R);
    if (!(zeta > 0.0f) || !std::isfinite(zeta)) return fail(GNNMP_EINVAL, "hyperbolic_graph: zeta = %g (not finite, or <= 0)", (double)zeta);
    // 2 cosh(zeta R), formed in double and rounded once (+inf above zeta R = 88.7: every pair with a finite value is then an edge)
    const float thr = (float)(2.0 * std::cosh((double)zeta * (double)R));
    // (dies when the call returns: after plan_build_long_rows' synchronisation, or its hipFree waits itself)
    DevBuf<HypNode> nodes;
    GNNMP_HIP(nodes.alloc((size_t)std::max<int64_t>(N, 1)));
    if (N > 0) {
        hyp_nodes_kernel<<<nblk(N), 256, 0, stream>>>(points, N, (double)zeta, nodes.get());
        GNNMP_HIP(hipGetLastError());
    }
    return threshold_graph<NB_HYP>("hyperbolic_graph", out, points, N, 2, thr, nodes.get(), graph_indicator, idx_bytes, index_base,
                                   n_graphs, self_loops, stream);
}

}  // extern "C"
