// topk.hip — TopKPool / topk_index      GraphNeuralNetworks/src/layers/pool.jl, GNNlib/src/layers/pool.jl:14-27
//   y   = p' * X / norm(p)                          gnnmp_topk_score_f32
//   idx = topk_index(y, k)                          gnnmp_topk_select_f32   (per member graph; keep flags for gnnmp_plan_keep_nodes)
//   X_  = view(X, :, idx) .* σ.(view(y, idx)')      gnnmp_topk_gate_f32, pullback gnnmp_topk_gate_grad_f32
// The reference pools ONE graph held as a dense matrix; here a batch is pooled member by member, and the child graph's plan is derived
// from the parent's by plan_edit.hip (gnnmp_plan_keep_nodes) with the keep flags this file writes.
//
// Selection is a RANK BY COUNTING on integer keys: key(v) is the monotone map of the fp32 bits to uint32 (-0.0 taken as +0.0, every
// NaN as key 0, below -Inf), and inside its member graph node i has
//   gt_i  = #{ j : key_j > key_i },   eqb_i = #{ j < i : key_j == key_i },   rank_i = gt_i + eqb_i
// — larger scores first, equal keys by ascending node id, NaNs last among themselves by id.  FIRST keeps rank_i < k_g, ALL keeps
// gt_i < k_g (every node whose key is at least the key of rank k_g - 1).  Integer compares and adds only: the counts do not depend on
// the order in which the j are visited, so the two routes below give the same words.
//   LDS route      a workgroup owns the member graphs that START inside its tile of TOPK_TILE nodes and fit the LDS budget; it loads
//                  the keys of a run of consecutive such graphs (as many as fit) into LDS and gives every node of the run one thread,
//                  which counts over the keys of its own graph.  A QM9-shaped batch (18 nodes a graph) packs ~14 graphs a workgroup.
//   device route   a member graph above the budget: every workgroup takes TOPK_TILE of its nodes and streams the graph's keys through
//                  a TOPK_CHUNK-key LDS window from device memory — n / TOPK_TILE workgroups a graph instead of one.
// Neither the host nor the launch shape knows the graph sizes (that would need a synchronisation): both kernels are launched over node
// tiles and find their work from graph_ptr.  O(n_g^2) compares a graph — see DESIGN.md §5 for where that loses to a sort.
//
// gnnmp_topk_select_radix_f32 writes the same keep words without the n^2: it finds the THRESHOLD key T of rank k_g - 1 by an MSD radix
// select over the 32-bit key (8 bits a pass, 4 passes) and keeps key > T, and of the nodes with key == T the first
// need = k_g - #{key > T} by node id (FIRST) or all of them (ALL).  Three routes by the node count n of a member graph:
//   small   n <= count_nodes             topk_lds_kernel above, unchanged: counting beats four passes at 20 keys a graph
//   mid     count_nodes < n <= lds_nodes  one workgroup a graph (the one that owns the 256-node tile the graph starts in): keys loaded
//                                        into LDS once; a pass is an LDS histogram of the keys that still match the prefix (integer
//                                        LDS atomics), a suffix scan of the 256 bins in one wave (four bins a lane, __shfl_down) and
//                                        the pick of the digit where the running count crosses the remaining k
//   tiled   n > lds_nodes                the batch's node range is cut into tiles of GNNMP_TOPK_RADIX_TILE nodes.  A pass is two launches:
//                                        every tile's workgroup stores the histogram of its keys of a tiled graph to the workspace; the
//                                        workgroup of the tile a graph STARTS in adds the graph's tile histograms, picks the digit and
//                                        stores (prefix, remaining k) beside that tile's histograms.  A last launch writes keep.
// eq_before_i = #{ j < i : key_j == T } is a ballot / popcount inside a wave, a walk over the wave totals inside a workgroup, and on the
// tiled route the sum of bin T & 255 of the last pass's histograms of the graph's earlier tiles (those bins ARE the tiles' counts of
// key == T).  Two invariants, not tuning: a tiled graph is longer than a tile (lds_nodes >= the tile), so a tile touches at most two of
// them — the tail of one (slot 0) and one that starts inside it (slot 1) — and at most one starts in a tile (its state slot).
//
// The row kernels (score, gate, gate pullback) give a row L lanes, L = the power of two >= min(C, 64): lane l takes the channels
// c = l, l + L, ... in ascending order, then the L partial sums fold in a butterfly (xor L/2, ..., 1).  No atomics anywhere.
#include <algorithm>
#include <cmath>

#include "common.h"

namespace gnnmp {
namespace {

constexpr int TOPK_BLOCK = 256;
constexpr int TOPK_TILE = 256;                      // nodes a workgroup owns (both routes)
constexpr int TOPK_CHUNK = 1024;                    // keys of the device route's LDS window
constexpr int64_t TOPK_LDS_DEFAULT = 1024;          // 256 keys: a 1024-node graph is 4x faster on the device route
constexpr int64_t TOPK_LDS_MAX = 64 * 1024;
constexpr int TOPK_GRAD_ROWS = GNNMP_TOPK_GRAD_ROWS;

inline unsigned nblk(int64_t n, int bs = TOPK_BLOCK) { return (unsigned)std::max<int64_t>(1, (n + bs - 1) / bs); }

// ---- selection -------------------------------------------------------------------------------------------------------------------------
struct TopkArgs {
    const float *score;
    const void *graph_ptr;
    int idx_bytes;
    int64_t G, N, k;
    double ratio;
    int ties;
    int64_t cap;            // keys of the LDS budget: member graphs of at most this many nodes take the LDS route
    uint32_t *keep;
    int32_t *rank;
};

__device__ __forceinline__ uint32_t topk_key(float v) {
    uint32_t u = __float_as_uint(v);
    if ((u & 0x7fffffffu) > 0x7f800000u) return 0u;      // NaN: after every number
    if (u == 0x80000000u) u = 0u;                         // -0.0 is +0.0
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
// node offset g of the batch, g in [0, G], clamped into [0, N] (a graph_ptr that does not ascend from 0 to N is the caller's error: the
// result is then undefined, but nothing is read or written outside the arrays and every loop ends)
__device__ __forceinline__ int64_t topk_bound(const TopkArgs &a, int64_t g) {
    if (!a.graph_ptr) return g <= 0 ? 0 : a.N;
    const int64_t v = load_index(a.graph_ptr, g, a.idx_bytes, 0);
    return v < 0 ? 0 : (v > a.N ? a.N : v);
}
// the last graph in [glo, ghi) that starts at or before node i (the graph that holds i when i lies in their range)
__device__ __forceinline__ int64_t topk_graph_of(const TopkArgs &a, int64_t i, int64_t glo, int64_t ghi) {
    while (ghi - glo > 1) {
        const int64_t mid = glo + (ghi - glo) / 2;
        if (topk_bound(a, mid) <= i) glo = mid; else ghi = mid;
    }
    return glo;
}
// keys[0 .. cnt) are the keys of nodes j0 .. j0 + cnt - 1
__device__ __forceinline__ void topk_count(uint32_t ki, int64_t i, const uint32_t *keys, int64_t j0, int cnt, uint32_t &gt, uint32_t &eqb) {
    for (int t = 0; t < cnt; ++t) {
        const uint32_t kj = keys[t];
        gt += kj > ki ? 1u : 0u;
        eqb += (kj == ki && j0 + t < i) ? 1u : 0u;
    }
}
// k_g of a member graph of n nodes (one definition for the counting and the radix export)
__device__ __forceinline__ int64_t topk_kg(const TopkArgs &a, int64_t n) {
    int64_t kg = a.k;
    if (a.k == 0) kg = (int64_t)ceil(a.ratio * (double)n);
    return kg > n ? n : kg;
}
__device__ __forceinline__ void topk_emit(const TopkArgs &a, int64_t i, int64_t n, uint32_t gt, uint32_t eqb) {
    const int64_t kg = topk_kg(a, n);
    const uint32_t rank = gt + eqb;
    a.keep[i] = (int64_t)(a.ties == GNNMP_TOPK_TIES_FIRST ? rank : gt) < kg ? 1u : 0u;
    if (a.rank) a.rank[i] = (int32_t)rank;
}

__global__ void __launch_bounds__(TOPK_BLOCK) topk_lds_kernel(const TopkArgs a) {
    extern __shared__ uint32_t topk_keys[];
    const int tid = threadIdx.x;
    if (blockIdx.x == 0 && tid == 0) a.keep[a.N] = 0u;      // closes the scan of gnnmp_plan_keep_nodes
    const int64_t tile_lo = (int64_t)blockIdx.x * TOPK_TILE, tile_hi = min(a.N, tile_lo + (int64_t)TOPK_TILE);
    // the first graph that starts at or after tile_lo (uniform over the workgroup, like everything up to the per-node loop)
    int64_t g = 0, ghi = a.G;
    while (g < ghi) {
        const int64_t mid = g + (ghi - g) / 2;
        if (topk_bound(a, mid) < tile_lo) g = mid + 1; else ghi = mid;
    }
    while (g < a.G) {
        const int64_t start = topk_bound(a, g);
        if (start >= tile_hi) break;
        int64_t end = topk_bound(a, g + 1);
        if (end - start > a.cap) {      // the device route's
            ++g;
            continue;
        }
        int64_t h = g + 1;              // the run g .. h - 1: graphs that start in the tile and whose keys fit together
        while (h < a.G) {
            const int64_t hs = topk_bound(a, h), he = topk_bound(a, h + 1);
            if (hs >= tile_hi || he < hs || he - start > a.cap) break;
            end = he;
            ++h;
        }
        const int cnt = (int)max((int64_t)0, end - start);
        for (int t = tid; t < cnt; t += TOPK_BLOCK) topk_keys[t] = topk_key(a.score[start + t]);
        __syncthreads();
        for (int t = tid; t < cnt; t += TOPK_BLOCK) {
            const int64_t i = start + t;
            const int64_t gi = topk_graph_of(a, i, g, h);
            const int64_t lo = max(start, topk_bound(a, gi)), hi = min(end, topk_bound(a, gi + 1));
            uint32_t gt = 0, eqb = 0;
            if (hi > lo) topk_count(topk_keys[t], i, topk_keys + (lo - start), lo, (int)(hi - lo), gt, eqb);
            topk_emit(a, i, hi - lo, gt, eqb);
        }
        __syncthreads();
        g = h;
    }
}

__global__ void __launch_bounds__(TOPK_BLOCK) topk_dev_kernel(const TopkArgs a) {
    __shared__ uint32_t s_keys[TOPK_CHUNK];
    const int tid = threadIdx.x;
    const int64_t tile_lo = (int64_t)blockIdx.x * TOPK_TILE, tile_hi = min(a.N, tile_lo + (int64_t)TOPK_TILE);
    if (tile_lo >= a.N) return;
    const int64_t i = tile_lo + tid;
    const uint32_t ki = i < a.N ? topk_key(a.score[i]) : 0u;
    const int64_t g_last = topk_graph_of(a, tile_hi - 1, 0, a.G);
    for (int64_t g = topk_graph_of(a, tile_lo, 0, a.G); g <= g_last; ++g) {      // the graphs with a node in the tile (uniform)
        const int64_t lo = topk_bound(a, g), hi = topk_bound(a, g + 1);
        if (hi - lo <= a.cap) continue;      // the LDS route's (and the empty ones)
        const bool mine = i < a.N && i >= lo && i < hi;
        uint32_t gt = 0, eqb = 0;
        for (int64_t c = lo; c < hi; c += TOPK_CHUNK) {
            const int cnt = (int)min((int64_t)TOPK_CHUNK, hi - c);
            for (int t = tid; t < cnt; t += TOPK_BLOCK) s_keys[t] = topk_key(a.score[c + t]);
            __syncthreads();
            if (mine) topk_count(ki, i, s_keys, c, cnt, gt, eqb);
            __syncthreads();
        }
        if (mine) topk_emit(a, i, hi - lo, gt, eqb);
    }
}

// ---- radix selection -------------------------------------------------------------------------------------------------------------------
constexpr int RADIX_TILE = GNNMP_TOPK_RADIX_TILE;   // nodes of a tile of the tiled route
constexpr int RADIX_BLOCK = 256;                    // threads of the tiled route's kernels: one a bin
constexpr int RADIX_MID_BLOCK = 1024;               // threads of the mid route's workgroup
constexpr int RADIX_BINS = 256;                     // 8 bits a pass
constexpr int RADIX_TILE_WORDS = 2 * RADIX_BINS + 4;      // workspace of a tile: histogram slot 0, slot 1, (prefix, remaining k, 0, 0)
constexpr int64_t RADIX_LDS_NODES = 15872;          // 62 KB of keys beside the 1.1 KB of static LDS: no opt-in above 64 KB is needed
static_assert(RADIX_BLOCK == RADIX_BINS && RADIX_TILE % RADIX_BLOCK == 0 && RADIX_LDS_NODES >= RADIX_TILE, "radix geometry");

struct RadixArgs {
    TopkArgs t;             // t.cap = count_nodes: the graphs of at most that many nodes are topk_lds_kernel's
    int64_t hi_n;           // lds_nodes (>= RADIX_TILE, >= t.cap): the graphs above it are the tiled route's
    uint32_t *ws;           // [n_tiles][RADIX_TILE_WORDS]
};

// wave 0, all 64 lanes: the digit d with #{keys in bins above d} < rem <= #{keys in bins d and above} -> sel[0] = d, sel[1] = rem - #{above}
__device__ __forceinline__ void radix_pick(const uint32_t *hist, uint32_t rem, int lane, uint32_t *sel) {
    uint32_t c[4], tot = 0;
    for (int q = 0; q < 4; ++q) {
        c[q] = hist[4 * lane + q];
        tot += c[q];
    }
    uint32_t v = tot;                                   // -> the count of the bins of this lane and of every higher lane
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t u = __shfl_down(v, o, 64);
        if (lane + o < 64) v += u;
    }
    uint32_t above = v - tot;
    if (lane == 0) {                                    // (only a graph_ptr that does not ascend leaves these in place)
        sel[0] = 0u;
        sel[1] = 1u;
    }
    for (int q = 3; q >= 0; --q) {
        if (above < rem && rem <= above + c[q]) {
            sel[0] = (uint32_t)(4 * lane + q);
            sel[1] = rem - above;
        }
        above += c[q];
    }
}
// one round of blockDim.x consecutive nodes, thread t the t-th: #{ earlier nodes of the graph with key == T } of this thread's node;
// base (the count of the rounds before, uniform) moves on by the round's total.  Every thread of the workgroup calls it: two barriers
template <int NW>
__device__ __forceinline__ uint32_t radix_eq_before(bool iseq, uint32_t *s_wtot, uint32_t &base) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long b = __ballot(iseq);
    if (lane == 0) s_wtot[wave] = (uint32_t)__popcll(b);
    __syncthreads();
    uint32_t before = base + (uint32_t)__popcll(b & ((1ull << lane) - 1ull)), total = 0;
    for (int w = 0; w < NW; ++w) {
        const uint32_t c = s_wtot[w];
        total += c;
        if (w < wave) before += c;
    }
    base += total;
    __syncthreads();
    return before;
}

// mid route: workgroup b owns the graphs of count_nodes < n <= lds_nodes that start in nodes [b * TOPK_TILE, (b + 1) * TOPK_TILE)
__global__ void __launch_bounds__(RADIX_MID_BLOCK) topk_radix_lds_kernel(const RadixArgs a) {
    extern __shared__ uint32_t radix_keys[];
    __shared__ uint32_t s_hist[RADIX_BINS], s_wtot[RADIX_MID_BLOCK / 64], s_sel[2];
    const TopkArgs &t = a.t;
    const int tid = threadIdx.x;
    const int64_t tile_lo = (int64_t)blockIdx.x * TOPK_TILE, tile_hi = min(t.N, tile_lo + (int64_t)TOPK_TILE);
    if (tile_lo >= t.N) return;
    int64_t g = 0, ghi = t.G;                           // the first graph that starts at or after tile_lo
    while (g < ghi) {
        const int64_t mid = g + (ghi - g) / 2;
        if (topk_bound(t, mid) < tile_lo) g = mid + 1; else ghi = mid;
    }
    // a graph longer than the tile that starts in it holds the tile's last node: the graphs before that one are the small route's
    if (t.cap >= TOPK_TILE) g = max(g, topk_graph_of(t, tile_hi - 1, 0, t.G));
    for (; g < t.G; ++g) {
        const int64_t start = topk_bound(t, g);
        if (start >= tile_hi) break;
        const int64_t n = topk_bound(t, g + 1) - start;
        if (n <= t.cap || n > a.hi_n) continue;
        const int cnt = (int)n;
        for (int i = tid; i < cnt; i += RADIX_MID_BLOCK) radix_keys[i] = topk_key(t.score[start + i]);
        uint32_t prefix = 0u, rem = (uint32_t)topk_kg(t, n);      // the key of rank rem - 1 among the keys that match prefix
        for (int shift = 24; shift >= 0; shift -= 8) {
            if (tid < RADIX_BINS) s_hist[tid] = 0u;
            __syncthreads();                            // (the keys are in LDS after the first of these)
            const uint32_t mask = shift == 24 ? 0u : 0xffffffffu << (shift + 8);
            for (int i = tid; i < cnt; i += RADIX_MID_BLOCK) {
                const uint32_t k = radix_keys[i];
                if ((k & mask) == prefix) atomicAdd(&s_hist[(k >> shift) & 255u], 1u);
            }
            __syncthreads();
            if (tid < 64) radix_pick(s_hist, rem, tid, s_sel);
            __syncthreads();
            prefix |= s_sel[0] << shift;
            rem = s_sel[1];
        }
        // prefix = T, rem = need = k_g - #{key > T} (1 <= need <= #{key == T})
        const bool first = t.ties == GNNMP_TOPK_TIES_FIRST;
        uint32_t base = 0u;
        for (int r0 = 0; r0 < cnt; r0 += RADIX_MID_BLOCK) {
            const int i = r0 + tid;
            const uint32_t k = i < cnt ? radix_keys[i] : 0u;
            const bool iseq = i < cnt && k == prefix;
            const uint32_t eqb = first ? radix_eq_before<RADIX_MID_BLOCK / 64>(iseq, s_wtot, base) : 0u;
            if (i < cnt) t.keep[start + i] = (k > prefix || (iseq && eqb < rem)) ? 1u : 0u;
        }
        __syncthreads();                                // the next graph's keys overwrite these
    }
}

// the tiled-route graph of a slot of the tile [tile_lo, tile_hi): slot 0 the graph that holds tile_lo and starts before it, slot 1 the
// graph that starts in the tile (longer than a tile, it holds the tile's last node).  false: the slot has none
__device__ __forceinline__ bool radix_span(const RadixArgs &a, int slot, int64_t tile_lo, int64_t tile_hi, int64_t &start, int64_t &end) {
    const int64_t g = topk_graph_of(a.t, slot ? tile_hi - 1 : tile_lo, 0, a.t.G);
    start = topk_bound(a.t, g);
    end = topk_bound(a.t, g + 1);
    return end - start > a.hi_n && (slot ? start >= tile_lo && start < tile_hi : start < tile_lo);
}
__device__ __forceinline__ uint32_t *radix_tile_ws(const RadixArgs &a, int64_t tile) { return a.ws + tile * RADIX_TILE_WORDS; }

// pass `shift` of the tiled route, first launch: ws[tile][slot][bin] = #{ nodes of the tile and of the slot's graph whose key matches the
// graph's prefix and has digit bin }.  Only the slots that have a graph are written, and only those are read
__global__ void __launch_bounds__(RADIX_BLOCK) topk_radix_hist_kernel(const RadixArgs a, int shift) {
    __shared__ uint32_t s_hist[2][RADIX_BINS];
    const int tid = threadIdx.x;
    const int64_t tile_lo = (int64_t)blockIdx.x * RADIX_TILE, tile_hi = min(a.t.N, tile_lo + (int64_t)RADIX_TILE);
    if (tile_lo >= a.t.N) return;
    s_hist[0][tid] = 0u;
    s_hist[1][tid] = 0u;
    __syncthreads();
    bool has[2];
    for (int slot = 0; slot < 2; ++slot) {
        int64_t start, end;
        has[slot] = radix_span(a, slot, tile_lo, tile_hi, start, end);
        if (!has[slot]) continue;
        uint32_t prefix = 0u, mask = 0u;
        if (shift != 24) {
            prefix = radix_tile_ws(a, start / RADIX_TILE)[2 * RADIX_BINS];
            mask = 0xffffffffu << (shift + 8);
        }
        const int64_t lo = max(start, tile_lo), hi = min(end, tile_hi);
        for (int64_t i = lo + tid; i < hi; i += RADIX_BLOCK) {
            const uint32_t k = topk_key(a.t.score[i]);
            if ((k & mask) == prefix) atomicAdd(&s_hist[slot][(k >> shift) & 255u], 1u);
        }
    }
    __syncthreads();
    for (int slot = 0; slot < 2; ++slot)
        if (has[slot]) radix_tile_ws(a, blockIdx.x)[slot * RADIX_BINS + tid] = s_hist[slot][tid];
}

// pass `shift`, second launch: the workgroup of the tile a tiled graph starts in adds the graph's tile histograms (ascending tiles: its
// own slot 1, then slot 0 of the tiles after it), picks the digit and stores (prefix, remaining k) in its tile's state words
__global__ void __launch_bounds__(RADIX_BLOCK) topk_radix_pick_kernel(const RadixArgs a, int shift) {
    __shared__ uint32_t s_hist[RADIX_BINS], s_sel[2];
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x, tile_lo = b * RADIX_TILE, tile_hi = min(a.t.N, tile_lo + (int64_t)RADIX_TILE);
    if (tile_lo >= a.t.N) return;
    int64_t start, end;
    if (!radix_span(a, 1, tile_lo, tile_hi, start, end)) return;
    uint32_t *state = radix_tile_ws(a, b) + 2 * RADIX_BINS;
    const uint32_t prefix = shift == 24 ? 0u : state[0], rem = shift == 24 ? (uint32_t)topk_kg(a.t, end - start) : state[1];
    const int64_t t_last = (end - 1) / RADIX_TILE;
    uint32_t c = radix_tile_ws(a, b)[RADIX_BINS + tid];
    for (int64_t tile = b + 1; tile <= t_last; ++tile) c += radix_tile_ws(a, tile)[tid];
    s_hist[tid] = c;
    __syncthreads();
    if (tid < 64) radix_pick(s_hist, rem, tid, s_sel);
    __syncthreads();
    if (tid == 0) {
        state[0] = prefix | (s_sel[0] << shift);
        state[1] = s_sel[1];
    }
}

// the tiled route's last launch: keep of the tile's nodes of its (at most two) tiled graphs from T and need in the graph's state words
__global__ void __launch_bounds__(RADIX_BLOCK) topk_radix_emit_kernel(const RadixArgs a) {
    __shared__ uint32_t s_wtot[RADIX_BLOCK / 64];
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x, tile_lo = b * RADIX_TILE, tile_hi = min(a.t.N, tile_lo + (int64_t)RADIX_TILE);
    if (tile_lo >= a.t.N) return;
    const bool first = a.t.ties == GNNMP_TOPK_TIES_FIRST;
    for (int slot = 0; slot < 2; ++slot) {
        int64_t start, end;
        if (!radix_span(a, slot, tile_lo, tile_hi, start, end)) continue;
        const int64_t st = start / RADIX_TILE;
        const uint32_t T = radix_tile_ws(a, st)[2 * RADIX_BINS], need = radix_tile_ws(a, st)[2 * RADIX_BINS + 1];
        uint32_t base = 0u;
        if (first) {
            // #{key == T} of the graph's earlier tiles: bin T & 255 of the last pass's histograms (thread t takes tiles st + t, + 256, ...;
            // then every thread holds the workgroup's sum)
            uint32_t part = 0u;
            for (int64_t tile = st + tid; tile < b; tile += RADIX_BLOCK)
                part += radix_tile_ws(a, tile)[(tile == st ? RADIX_BINS : 0) + (T & 255u)];
            for (int o = 32; o >= 1; o >>= 1) part += __shfl_xor(part, o, 64);
            if ((tid & 63) == 0) s_wtot[tid >> 6] = part;
            __syncthreads();
            for (int w = 0; w < RADIX_BLOCK / 64; ++w) base += s_wtot[w];
            __syncthreads();
        }
        const int64_t lo = max(start, tile_lo), hi = min(end, tile_hi);
        for (int64_t r0 = lo; r0 < hi; r0 += RADIX_BLOCK) {
            const int64_t i = r0 + tid;
            const uint32_t k = i < hi ? topk_key(a.t.score[i]) : 0u;
            const bool iseq = i < hi && k == T;
            const uint32_t eqb = first ? radix_eq_before<RADIX_BLOCK / 64>(iseq, s_wtot, base) : 0u;
            if (i < hi) a.t.keep[i] = (k > T || (iseq && eqb < need)) ? 1u : 0u;
        }
    }
}

// ---- the row kernels -------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float group_sum(float v, int L) {
    for (int o = L >> 1; o >= 1; o >>= 1) v = v + __shfl_xor(v, o, 64);
    return v;
}
// sqrt(sum p^2): lane l adds its channels in ascending order, then the butterfly — the same on every lane of the group
__device__ __forceinline__ float group_norm(const float *__restrict__ p, int64_t C, int lane, int L) {
    float s = 0.0f;
    for (int64_t c = lane; c < C; c += L) s = s + p[c] * p[c];
    return sqrtf(group_sum(s, L));
}
inline int lanes_of(int64_t C) {
    int L = 1;
    while (L < 64 && L < C) L <<= 1;
    return L;
}

__global__ void __launch_bounds__(TOPK_BLOCK) topk_score_kernel(const float *__restrict__ x, const float *__restrict__ p, float *__restrict__ y,
                                                                int64_t N, int64_t C, int L) {
    const int lane = threadIdx.x & (L - 1);
    const int64_t i = ((int64_t)blockIdx.x * TOPK_BLOCK + threadIdx.x) / L;
    const float norm = group_norm(p, C, lane, L);
    float s = 0.0f;
    if (i < N)
        for (int64_t c = lane; c < C; c += L) s = s + p[c] * x[i * C + c];
    s = group_sum(s, L);
    if (i < N && lane == 0) y[i] = s / norm;
}

// g = act(y) and act'(y)
__device__ __forceinline__ float topk_act(int act, float y, float &dg) {
    if (act == GNNMP_TOPK_ACT_SIGMOID) {
        const float g = 1.0f / (1.0f + expf(-y));
        dg = g * (1.0f - g);
        return g;
    }
    if (act == GNNMP_TOPK_ACT_TANH) {
        const float g = tanhf(y);
        dg = 1.0f - g * g;
        return g;
    }
    dg = 1.0f;
    return y;
}

// element e of out [n_keep][C] (VEC = 4: four of them; C % 4 == 0 and both arrays 16-byte aligned)
template <int VEC>
__global__ void __launch_bounds__(TOPK_BLOCK) topk_gate_kernel(const float *__restrict__ x, const float *__restrict__ y,
                                                               const int32_t *__restrict__ node_map, int act, float *__restrict__ out,
                                                               int64_t total, int64_t Cv) {
    const int64_t e = (int64_t)blockIdx.x * TOPK_BLOCK + threadIdx.x;
    if (e >= total) return;
    const int64_t r = e / Cv, c = e - r * Cv, i = node_map[r];
    float dg;
    const float g = topk_act(act, y[i], dg);
    if (VEC == 4) {
        float4 v = reinterpret_cast<const float4 *>(x)[i * Cv + c];
        v.x = v.x * g; v.y = v.y * g; v.z = v.z * g; v.w = v.w * g;
        reinterpret_cast<float4 *>(out)[e] = v;
    } else {
        out[e] = x[i * Cv + c] * g;
    }
}

struct GradArgs {
    const float *x, *y, *p, *dout;
    const int32_t *node_new;
    int act, L;
    int64_t N, C;
    float *dx, *dy, *part;
    int want_part;
};
// workgroup b walks the parent's rows b * TOPK_GRAD_ROWS ..: every row L lanes; then, for dp, thread c adds dy_i * x[i][c] over the
// workgroup's kept rows in ascending i (column C: dy_i * y_i) into part[b][c]
__global__ void __launch_bounds__(TOPK_BLOCK) topk_gate_grad_kernel(const GradArgs a) {
    __shared__ float s_dy[TOPK_GRAD_ROWS];
    __shared__ int s_kept[TOPK_GRAD_ROWS];
    const int L = a.L, tid = threadIdx.x, lane = tid & (L - 1), grp = tid / L, ngrp = TOPK_BLOCK / L;
    const int64_t row0 = (int64_t)blockIdx.x * TOPK_GRAD_ROWS, C = a.C;
    const float norm = a.p ? group_norm(a.p, C, lane, L) : 1.0f;
    for (int rr = grp; rr < TOPK_GRAD_ROWS; rr += ngrp) {      // (whole waves leave together: 64 rows, ngrp a power of two)
        const int64_t i = row0 + rr;
        const bool valid = i < a.N;
        const int64_t r = valid ? (int64_t)a.node_new[i] : -1;
        float s = 0.0f;
        if (r >= 0)
            for (int64_t c = lane; c < C; c += L) s = s + a.dout[r * C + c] * a.x[i * C + c];
        s = group_sum(s, L);
        float g = 0.0f, dyi = 0.0f;
        if (r >= 0) {
            float dg;
            g = topk_act(a.act, a.y[i], dg);
            dyi = dg * s;
        }
        if (valid) {
            for (int64_t c = lane; c < C; c += L) {
                float v = 0.0f;
                if (r >= 0) {
                    v = a.dout[r * C + c] * g;
                    if (a.p) v = v + (dyi * a.p[c]) / norm;
                }
                a.dx[i * C + c] = v;
            }
            if (lane == 0 && a.dy) a.dy[i] = dyi;
        }
        if (lane == 0) {
            s_dy[rr] = dyi;
            s_kept[rr] = r >= 0 ? 1 : 0;
        }
    }
    if (!a.want_part) return;
    __syncthreads();
    const int nrows = (int)min((int64_t)TOPK_GRAD_ROWS, a.N - row0);
    for (int64_t c = tid; c <= C; c += TOPK_BLOCK) {
        float acc = 0.0f;
        for (int rr = 0; rr < nrows; ++rr)
            if (s_kept[rr]) acc = acc + s_dy[rr] * (c < C ? a.x[(row0 + rr) * C + c] : a.y[row0 + rr]);
        a.part[(int64_t)blockIdx.x * (C + 1) + c] = acc;
    }
}
// dp[c] = A_c / norm - B * p[c] / norm^2 with A_c = sum_b part[b][c], B = sum_b part[b][C], both in ascending b; norm^2 = sum p^2 in
// ascending c (every thread adds all three itself)
__global__ void __launch_bounds__(TOPK_BLOCK) topk_gate_fold_kernel(const float *__restrict__ part, const float *__restrict__ p,
                                                                    float *__restrict__ dp, int64_t nb, int64_t C) {
    const int64_t c = (int64_t)blockIdx.x * TOPK_BLOCK + threadIdx.x;
    if (c >= C) return;
    float A = 0.0f, B = 0.0f, n2 = 0.0f;
    for (int64_t b = 0; b < nb; ++b) {
        A = A + part[b * (C + 1) + c];
        B = B + part[b * (C + 1) + C];
    }
    for (int64_t j = 0; j < C; ++j) n2 = n2 + p[j] * p[j];
    dp[c] = A / sqrtf(n2) - (B * p[c]) / n2;
}

inline bool bad_act(int act) { return act != GNNMP_TOPK_ACT_SIGMOID && act != GNNMP_TOPK_ACT_TANH && act != GNNMP_TOPK_ACT_IDENTITY; }
inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace
}  // namespace gnnmp

using namespace gnnmp;

extern "C" {

int gnnmp_topk_score_f32(const float *x, const float *p, float *y, int64_t N, int64_t C, gnnmp_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (N < 0 || C < 1) return fail(GNNMP_EINVAL, "topk_score: N = %lld, C = %lld", (long long)N, (long long)C);
    if (N >= (int64_t)INT32_MAX) return fail(GNNMP_EUNSUPPORTED, "topk_score: N = %lld (limit 2^31 - 2)", (long long)N);
    if (!p || (N > 0 && (!x || !y))) return fail(GNNMP_EINVAL, "topk_score: NULL x, p or y");
    if (N == 0) return GNNMP_OK;
    const int L = lanes_of(C);
    topk_score_kernel<<<nblk(N * L), TOPK_BLOCK, 0, stream>>>(x, p, y, N, C, L);
    GNNMP_LAUNCH_CHECK("topk_score_kernel");
    return GNNMP_OK;
}

int gnnmp_topk_select_f32(const gnnmp_topk_t *job, int64_t N, gnnmp_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!job) return fail(GNNMP_EINVAL, "topk_select: null job");
    if (N < 0) return fail(GNNMP_EINVAL, "topk_select: negative N");
    if (N >= (int64_t)INT32_MAX) return fail(GNNMP_EUNSUPPORTED, "topk_select: N = %lld (limit 2^31 - 2)", (long long)N);
    if (job->idx_bytes != 4 && job->idx_bytes != 8) return fail(GNNMP_EINVAL, "topk_select: idx_bytes %d", job->idx_bytes);
    if (job->graph_ptr && job->n_graphs < 1) return fail(GNNMP_EINVAL, "topk_select: n_graphs %lld with a graph_ptr", (long long)job->n_graphs);
    if (job->k < 0) return fail(GNNMP_EINVAL, "topk_select: k = %lld (k >= 1, or 0 with a ratio)", (long long)job->k);
    if (job->k == 0 && !(job->ratio > 0.0f && job->ratio <= 1.0f))
        return fail(GNNMP_EINVAL, "topk_select: ratio %g outside (0, 1]", (double)job->ratio);
    if (job->ties != GNNMP_TOPK_TIES_FIRST && job->ties != GNNMP_TOPK_TIES_ALL) return fail(GNNMP_EINVAL, "topk_select: ties %d", job->ties);
    if (job->lds_budget_bytes < 0) return fail(GNNMP_EINVAL, "topk_select: negative lds_budget_bytes");
    if (!job->keep) return fail(GNNMP_EINVAL, "topk_select: null keep");
    if (N > 0 && !job->score) return fail(GNNMP_EINVAL, "topk_select: null score");
    TopkArgs a;
    a.score = job->score;
    a.graph_ptr = job->graph_ptr;
    a.idx_bytes = job->idx_bytes;
    a.G = job->graph_ptr ? job->n_graphs : 1;
    a.N = N;
    a.k = job->k;
    a.ratio = (double)job->ratio;
    a.ties = job->ties;
    a.cap = std::max<int64_t>(1, std::min(job->lds_budget_bytes == 0 ? TOPK_LDS_DEFAULT : job->lds_budget_bytes, TOPK_LDS_MAX) / 4);
    a.keep = job->keep;
    a.rank = job->rank;
    // one graph: its size is known here, so only its route is launched (the LDS kernel always is: it closes keep[N])
    const bool one_large = !job->graph_ptr && N > a.cap;
    if (one_large) a.cap = 0;
    topk_lds_kernel<<<one_large ? 1u : nblk(N, TOPK_TILE), TOPK_BLOCK, (size_t)std::max<int64_t>(a.cap, 1) * sizeof(uint32_t), stream>>>(a);
    GNNMP_LAUNCH_CHECK("topk_lds_kernel");
    if (N > a.cap) {      // some member graph may be above the budget
        topk_dev_kernel<<<nblk(N, TOPK_TILE), TOPK_BLOCK, 0, stream>>>(a);
        GNNMP_LAUNCH_CHECK("topk_dev_kernel");
    }
    return GNNMP_OK;
}

int64_t gnnmp_topk_select_radix_workspace(int64_t N) {
    if (N <= (int64_t)RADIX_TILE) return 0;      // no graph is longer than a tile: none is on the tiled route
    return (N + RADIX_TILE - 1) / RADIX_TILE * (int64_t)(RADIX_TILE_WORDS * sizeof(uint32_t));
}

int gnnmp_topk_select_radix_f32(const gnnmp_topk_radix_t *job, int64_t N, gnnmp_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!job) return fail(GNNMP_EINVAL, "topk_select_radix: null job");
    if (N < 0) return fail(GNNMP_EINVAL, "topk_select_radix: negative N");
    if (N >= (int64_t)INT32_MAX) return fail(GNNMP_EUNSUPPORTED, "topk_select_radix: N = %lld (limit 2^31 - 2)", (long long)N);
    if (job->idx_bytes != 4 && job->idx_bytes != 8) return fail(GNNMP_EINVAL, "topk_select_radix: idx_bytes %d", job->idx_bytes);
    if (job->graph_ptr && job->n_graphs < 1)
        return fail(GNNMP_EINVAL, "topk_select_radix: n_graphs %lld with a graph_ptr", (long long)job->n_graphs);
    if (job->k < 0) return fail(GNNMP_EINVAL, "topk_select_radix: k = %lld (k >= 1, or 0 with a ratio)", (long long)job->k);
    if (job->k == 0 && !(job->ratio > 0.0f && job->ratio <= 1.0f))
        return fail(GNNMP_EINVAL, "topk_select_radix: ratio %g outside (0, 1]", (double)job->ratio);
    if (job->ties != GNNMP_TOPK_TIES_FIRST && job->ties != GNNMP_TOPK_TIES_ALL)
        return fail(GNNMP_EINVAL, "topk_select_radix: ties %d", job->ties);
    if (job->count_nodes < 0 || job->lds_nodes < 0)
        return fail(GNNMP_EINVAL, "topk_select_radix: negative count_nodes or lds_nodes");
    if (!job->keep) return fail(GNNMP_EINVAL, "topk_select_radix: null keep");
    if (N > 0 && !job->score) return fail(GNNMP_EINVAL, "topk_select_radix: null score");
    RadixArgs a;
    a.t.score = job->score;
    a.t.graph_ptr = job->graph_ptr;
    a.t.idx_bytes = job->idx_bytes;
    a.t.G = job->graph_ptr ? job->n_graphs : 1;
    a.t.N = N;
    a.t.k = job->k;
    a.t.ratio = (double)job->ratio;
    a.t.ties = job->ties;
    a.t.cap = job->count_nodes == 0 ? TOPK_LDS_DEFAULT / 4 : std::min(job->count_nodes, TOPK_LDS_MAX / 4);
    a.t.keep = job->keep;
    a.t.rank = nullptr;
    a.hi_n = job->lds_nodes == 0 ? RADIX_LDS_NODES : std::min(std::max<int64_t>(job->lds_nodes, RADIX_TILE), RADIX_LDS_NODES);
    a.hi_n = std::max(a.hi_n, a.t.cap);          // (every size has exactly one route)
    a.ws = job->workspace;
    const bool tiled = N > a.hi_n;               // some member graph may be on the tiled route
    if (tiled && (!job->workspace || job->workspace_bytes < gnnmp_topk_select_radix_workspace(N)))
        return fail(GNNMP_EINVAL, "topk_select_radix: workspace %s, %lld bytes (N = %lld needs %lld)", job->workspace ? "given" : "NULL",
                    (long long)job->workspace_bytes, (long long)N, (long long)gnnmp_topk_select_radix_workspace(N));
    // one graph: its size is known here, so only its route is launched (the counting kernel always is: it closes keep[N])
    const bool one = !job->graph_ptr;
    TopkArgs small = a.t;
    if (one && N > a.t.cap) small.cap = 0;
    topk_lds_kernel<<<one ? 1u : nblk(N, TOPK_TILE), TOPK_BLOCK, (size_t)std::max<int64_t>(small.cap, 1) * sizeof(uint32_t), stream>>>(small);
    GNNMP_LAUNCH_CHECK("topk_lds_kernel");
    if (N > a.t.cap && !(one && tiled)) {
        topk_radix_lds_kernel<<<one ? 1u : nblk(N, TOPK_TILE), RADIX_MID_BLOCK, (size_t)std::min(a.hi_n, N) * sizeof(uint32_t), stream>>>(a);
        GNNMP_LAUNCH_CHECK("topk_radix_lds_kernel");
    }
    if (tiled) {
        const unsigned tiles = nblk(N, RADIX_TILE);
        for (int shift = 24; shift >= 0; shift -= 8) {
            topk_radix_hist_kernel<<<tiles, RADIX_BLOCK, 0, stream>>>(a, shift);
            GNNMP_LAUNCH_CHECK("topk_radix_hist_kernel");
            topk_radix_pick_kernel<<<tiles, RADIX_BLOCK, 0, stream>>>(a, shift);
            GNNMP_LAUNCH_CHECK("topk_radix_pick_kernel");
        }
        topk_radix_emit_kernel<<<tiles, RADIX_BLOCK, 0, stream>>>(a);
        GNNMP_LAUNCH_CHECK("topk_radix_emit_kernel");
    }
    return GNNMP_OK;
}

int gnnmp_topk_gate_f32(const gnnmp_topk_gate_t *job, int64_t n_keep, int64_t C, gnnmp_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!job) return fail(GNNMP_EINVAL, "topk_gate: null job");
    if (n_keep < 0 || C < 1) return fail(GNNMP_EINVAL, "topk_gate: n_keep = %lld, C = %lld", (long long)n_keep, (long long)C);
    if (bad_act(job->act)) return fail(GNNMP_EINVAL, "topk_gate: act %d", job->act);
    if (n_keep > 0 && (!job->x || !job->y || !job->node_map || !job->out)) return fail(GNNMP_EINVAL, "topk_gate: NULL x, y, node_map or out");
    if (n_keep == 0) return GNNMP_OK;
    if (C % 4 == 0 && aligned16(job->x) && aligned16(job->out)) {
        const int64_t total = n_keep * (C / 4);
        topk_gate_kernel<4><<<nblk(total), TOPK_BLOCK, 0, stream>>>(job->x, job->y, job->node_map, job->act, job->out, total, C / 4);
    } else {
        const int64_t total = n_keep * C;
        topk_gate_kernel<1><<<nblk(total), TOPK_BLOCK, 0, stream>>>(job->x, job->y, job->node_map, job->act, job->out, total, C);
    }
    GNNMP_LAUNCH_CHECK("topk_gate_kernel");
    return GNNMP_OK;
}

int gnnmp_topk_gate_grad_f32(const gnnmp_topk_gate_grad_t *job, int64_t N, int64_t C, gnnmp_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!job) return fail(GNNMP_EINVAL, "topk_gate_grad: null job");
    if (N < 0 || C < 1) return fail(GNNMP_EINVAL, "topk_gate_grad: N = %lld, C = %lld", (long long)N, (long long)C);
    if (bad_act(job->act)) return fail(GNNMP_EINVAL, "topk_gate_grad: act %d", job->act);
    if (job->dp && (!job->p || !job->part)) return fail(GNNMP_EINVAL, "topk_gate_grad: dp needs p and part");
    if (N > 0 && (!job->x || !job->y || !job->dout || !job->node_new || !job->dx))
        return fail(GNNMP_EINVAL, "topk_gate_grad: NULL x, y, dout, node_new or dx");
    const int64_t nb = (N + TOPK_GRAD_ROWS - 1) / TOPK_GRAD_ROWS;
    if (N > 0) {
        GradArgs a;
        a.x = job->x; a.y = job->y; a.p = job->p; a.dout = job->dout;
        a.node_new = job->node_new;
        a.act = job->act;
        a.L = lanes_of(C);
        a.N = N; a.C = C;
        a.dx = job->dx; a.dy = job->dy; a.part = job->part;
        a.want_part = job->dp ? 1 : 0;
        topk_gate_grad_kernel<<<(unsigned)nb, TOPK_BLOCK, 0, stream>>>(a);
        GNNMP_LAUNCH_CHECK("topk_gate_grad_kernel");
    }
    if (job->dp) {
        topk_gate_fold_kernel<<<nblk(C), TOPK_BLOCK, 0, stream>>>(job->part, job->p, job->dp, nb, C);
        GNNMP_LAUNCH_CHECK("topk_gate_fold_kernel");
    }
    return GNNMP_OK;
}

}  // extern "C"
