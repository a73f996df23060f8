// linkpred.hip — link prediction (GraphNeuralNetworks/examples/link_prediction_pubmed.jl) on the device:
//   negative_sample(g; num_neg_edges, bidirected)   GNNGraphs/src/transform.jl:890-929
//   rand_edge_split(g, frac; bidirected)            GNNGraphs/src/transform.jl:945-968
//   the adjoint of apply_edges(xi_dot_xj, g, xi, xj) w.r.t. the node features (DotDecoder, GNNlib/src/layers/basic.jl:1-3)
// The reference runs the two graph transforms on the CPU (edge_index copied to the host and back on every call).
#include <algorithm>
#include <cmath>

#include "slotwalk.h"
#include "scratch.h"
#include "sort_scan.h"

namespace gnnmp {
namespace {

inline unsigned nblk(int64_t n, int bs = 256) { return (unsigned)((n + bs - 1) / bs); }

// the counter-based generator of graphprep.hip (splitmix64 finaliser)
__device__ __forceinline__ uint64_t lp_mix64(uint64_t z) {
    z += 0x9e3779b97f4a7c15ULL;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
    return z ^ (z >> 31);
}
// uniform in (0, 1]: log(u) stays finite
__device__ __forceinline__ double lp_uniform_open0(uint64_t stream, uint64_t draw) {
    const uint64_t r = lp_mix64(stream + draw);
    return (double)((r >> 11) + 1) * (1.0 / 9007199254740992.0);
}

// first position of a sorted array holding a value >= key
__device__ __forceinline__ int64_t lower_bound_u64(const uint64_t *a, int64_t n, uint64_t key) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (a[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// ---- negative_sample -------------------------------------------------------------------------------------------------
// 0-based code of edge (s, t): s n + t (the reference's (s-1) n + t, minus one).  bad[0] = 1 for an index outside 0..n-1.
__global__ void edge_codes_kernel(const void *s, const void *t, int idx_bytes, int base, int64_t E, int64_t n, uint64_t *codes,
                                  int *bad) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= E) return;
    const int64_t a = load_index(s, k, idx_bytes, base), b = load_index(t, k, idx_bytes, base);
    if (a < 0 || b < 0 || a >= n || b >= n) {
        *bad = 1;
        codes[k] = 0;
        return;
    }
    codes[k] = (uint64_t)a * (uint64_t)n + (uint64_t)b;
}

struct NegTrialArgs {
    const uint64_t *pos;    // sorted codes of g's edges (self loops are rejected arithmetically, not looked up)
    int64_t n_pos;
    const uint64_t *prev;   // sorted codes kept by the earlier trials
    int64_t n_prev;
    uint64_t maxid, chunk_len, n1;   // n^2, codes per chunk, n + 1
    int64_t n_chunks;
    uint64_t stream;        // this trial's stream key
    double log1m_p;         // log1p(-p) (< 0); p_one: every code is a candidate
    int p_one;
    int64_t *counts;        // WRITE = 0: kept candidates of every chunk
    const int64_t *offsets; // WRITE = 1: exclusive prefix sums of counts
    uint64_t *out;          // WRITE = 1: out[offsets[c] + j] for offsets[c] + j < room
    int64_t room;
};

// One thread per chunk of the code space [c L, min((c + 1) L, n^2)).  randsubseq(1:maxid, p) restricted to the chunk is a walk by
// geometric gaps: P(gap >= k) = (1 - p)^k for gap = floor(log(u) / log1p(-p)), u uniform in (0, 1] — exactly one Bernoulli(p) draw
// per code, and the chunk's draws form their own counter-based stream (the count and write passes walk the same candidates).  A
// candidate is kept unless it is a self loop (c mod (n + 1) = 0), an edge of g, or a code an earlier trial kept: setdiff! against
// the positives, then union! (transform.jl:915-917).  The candidates of a chunk ascend, and so do both sorted lists, so each is one
// binary search at the chunk's start and then a forward merge: O(candidates + positives) work over the whole grid, never O(n^2).
template <int WRITE>
__global__ void __launch_bounds__(256) neg_trial_kernel(const NegTrialArgs a) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.n_chunks) return;
    const uint64_t lo = (uint64_t)c * a.chunk_len;
    const uint64_t hi = min(lo + a.chunk_len, a.maxid);
    const uint64_t stream = lp_mix64(a.stream ^ ((uint64_t)c * 0xd1342543de82ef95ULL));
    int64_t ip = lower_bound_u64(a.pos, a.n_pos, lo);
    int64_t iq = a.n_prev ? lower_bound_u64(a.prev, a.n_prev, lo) : 0;
    int64_t kept = 0, o = 0;
    if (WRITE) o = a.offsets[c];
    uint64_t cur = lo;   // first code not yet decided
    for (uint64_t draw = 0;; ++draw) {
        uint64_t code;
        if (a.p_one) {
            code = cur;
        } else {
            const double gap = floor(log(lp_uniform_open0(stream, draw)) / a.log1m_p);
            if (!(gap < (double)(hi - cur))) break;   // (also stops on a gap beyond 2^64)
            code = cur + (uint64_t)gap;
        }
        if (code >= hi) break;
        cur = code + 1;
        if (code % a.n1 == 0) continue;                                   // self loop (s, s): a positive
        while (ip < a.n_pos && a.pos[ip] < code) ++ip;
        if (ip < a.n_pos && a.pos[ip] == code) continue;                  // an edge of g
        while (iq < a.n_prev && a.prev[iq] < code) ++iq;
        if (iq < a.n_prev && a.prev[iq] == code) continue;                // kept by an earlier trial
        if (WRITE) {
            if (o + kept >= a.room) break;                                // truncated: idx_neg[1:num_neg_edges]
            a.out[o + kept] = code;
        }
        ++kept;
    }
    if (!WRITE) a.counts[c] = kept;
}

// decode the kept codes: s = c / n, t = c % n (edge_decoding, utils.jl:230-233); bidirected: [s; t], [t; s]
__global__ void neg_decode_kernel(const uint64_t *codes, int64_t k, uint64_t n, int bidirected, int idx_bytes, int base, void *s_out,
                                  void *t_out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= k) return;
    const int64_t s = (int64_t)(codes[i] / n), t = (int64_t)(codes[i] % n);
    store_index(s_out, i, idx_bytes, s + base);
    store_index(t_out, i, idx_bytes, t + base);
    if (bidirected) {
        store_index(s_out, k + i, idx_bytes, t + base);
        store_index(t_out, k + i, idx_bytes, s + base);
    }
}

static int bit_length(uint64_t v) {
    int b = 0;
    while (v) {
        ++b;
        v >>= 1;
    }
    return b;
}

// ---- rand_edge_split -------------------------------------------------------------------------------------------------
__global__ void less_flag_kernel(const void *s, const void *t, int idx_bytes, int64_t E, int64_t *flags) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k > E) return;
    flags[k] = k < E && load_index(s, k, idx_bytes, 0) < load_index(t, k, idx_bytes, 0) ? 1 : 0;
}
// kept[pos[k]] = k for the edges with s < t, the first `ne` of them (in edge order)
__global__ void less_compact_kernel(const int64_t *flags, const int64_t *pos, int64_t E, int64_t ne, int64_t *kept) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= E || !flags[k] || pos[k] >= ne) return;
    kept[pos[k]] = k;
}
// key of position i: `rbits` random bits above the `ibits` bits of i.  Sorted, the low bits are a uniformly random permutation of
// 0..ne-1 (keys that tie on the random bits keep index order: a pair of equal draws has probability ne^2 / 2^(rbits + 1)).
__global__ void perm_keys_kernel(int64_t ne, int ibits, uint64_t seed, uint64_t *keys) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ne) return;
    const uint64_t r = lp_mix64(lp_mix64(seed) + (uint64_t)i);
    keys[i] = ibits >= 64 ? (uint64_t)i : (((r >> ibits) << ibits) | (uint64_t)i);
}
__global__ void split_write_kernel(const uint64_t *sorted, int ibits, const int64_t *kept, const void *s, const void *t, int idx_bytes,
                                   int64_t ne, int64_t size1, int bidirected, void *s1, void *t1, void *s2, void *t2) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ne) return;
    const uint64_t mask = ibits >= 64 ? ~0ULL : ((1ULL << ibits) - 1ULL);
    int64_t e = (int64_t)(sorted[i] & mask);
    if (kept) e = kept[e];
    const int64_t a = load_index(s, e, idx_bytes, 0), b = load_index(t, e, idx_bytes, 0);   // raw values: width and base kept
    void *so = i < size1 ? s1 : s2, *to = i < size1 ? t1 : t2;
    const int64_t j = i < size1 ? i : i - size1, m = i < size1 ? size1 : ne - size1;
    store_index(so, j, idx_bytes, a);
    store_index(to, j, idx_bytes, b);
    if (bidirected) {                 // [s1; t1], [t1; s1]
        store_index(so, m + j, idx_bytes, b);
        store_index(to, m + j, idx_bytes, a);
    }
}

// ---- the adjoint of the per-edge dot product -------------------------------------------------------------------------------
// z_k = <xi[t_k], xj[s_k]>:  dxi[v] = Σ_{k: t_k = v} dz_k xj[s_k]  (the plan's row v),  dxj[u] = Σ_{k: s_k = u} dz_k xi[t_k]  (the
// transposed plan's row u).  A group of G lanes owns a destination row, each lane NT feature tiles of VEC floats; the row's slots are
// walked in plan order (original edge order) with the sum in registers and written once: no atomics, no partials, a fixed order.
// Products are rounded before the add (-ffp-contract=off), the arithmetic of propagate(w_mul_xj) with w = dz.
struct EdgeDotGradArgs {
    const uint32_t *rowptr, *rowptr_t;
    const int32_t *col, *eid, *col_t, *eid_t;
    const float *xi, *xj, *dz;
    float *dxi, *dxj;   // alias mode: dxi == dxj, one row = in-edge sum + out-edge sum
    int alias;
    int D, n_rows, waves;
};

template <int VEC, int NT, int G, int U>
__device__ __forceinline__ void row_accumulate(const uint32_t *rowptr, const int32_t *col, const int32_t *eid, const float *x,
                                               const float *dz, int row, int D, int lig, int gbase, float (&acc)[NT][VEC]) {
    const uint32_t beg = rowptr[row], end = rowptr[row + 1];
    for (uint32_t base = beg; base < end; base += G) {
        const Slots s = load_slots<true, true>(col, eid, base, end, lig, G);
        const float w = base + lig < end ? dz[s.ev] : 0.0f;
        for (int j = 0; j < s.n; j += U) {
            float xv[U][NT][VEC];
            float wv[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {      // the broadcast stays here, slot by slot with its loads: bcast_word ahead of the loop
                const int src = gbase + min(j + u, s.n - 1);      // costs one instance a wave (LABNOTES.md)
                const int cj = __shfl(s.c, src, 64);
                wv[u] = __shfl(w, src, 64);
#pragma unroll
                for (int tl = 0; tl < NT; ++tl) {
                    const int f = (tl * G + lig) * VEC;
                    load_or_zero<VEC>(f < D, x + (int64_t)cj * D + f, xv[u][tl]);
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (j + u < s.n) {
#pragma unroll
                    for (int tl = 0; tl < NT; ++tl)
#pragma unroll
                        for (int q = 0; q < VEC; ++q) acc[tl][q] += wv[u] * xv[u][tl][q];
                }
            }
        }
    }
}

template <int VEC, int LOG2G, int NT>
__global__ void __launch_bounds__(256) edge_dot_grad_kernel(const EdgeDotGradArgs a) {
    constexpr int G = 1 << LOG2G;
    constexpr int U0 = NT == 1 ? 8 : (NT == 2 ? 4 : 2);   // slots in flight per lane
    constexpr int U = U0 < G ? U0 : G;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int lig = lane & (G - 1);
    const int gbase = lane - lig;
    constexpr int rpw = 64 >> LOG2G;
    const int64_t v64 = ((int64_t)blockIdx.x * a.waves + wave) * rpw + (lane >> LOG2G);
    const int64_t n_virtual = a.alias ? a.n_rows : 2 * (int64_t)a.n_rows;
    if (v64 >= n_virtual) return;   // (whole groups leave together: the shuffles stay inside live groups)
    const bool second = v64 >= a.n_rows;      // split mode: rows n..2n-1 are dxj's
    const int row = (int)(second ? v64 - a.n_rows : v64);
    float acc[NT][VEC];
#pragma unroll
    for (int tl = 0; tl < NT; ++tl)
#pragma unroll
        for (int q = 0; q < VEC; ++q) acc[tl][q] = 0.0f;
    float *out;
    if (a.alias) {
        float acc2[NT][VEC];
#pragma unroll
        for (int tl = 0; tl < NT; ++tl)
#pragma unroll
            for (int q = 0; q < VEC; ++q) acc2[tl][q] = 0.0f;
        row_accumulate<VEC, NT, G, U>(a.rowptr, a.col, a.eid, a.xj, a.dz, row, a.D, lig, gbase, acc);
        row_accumulate<VEC, NT, G, U>(a.rowptr_t, a.col_t, a.eid_t, a.xi, a.dz, row, a.D, lig, gbase, acc2);
#pragma unroll
        for (int tl = 0; tl < NT; ++tl)
#pragma unroll
            for (int q = 0; q < VEC; ++q) acc[tl][q] = acc[tl][q] + acc2[tl][q];   // (in-edge sum) + (out-edge sum)
        out = a.dxi;
    } else if (!second) {
        if (!a.dxi) return;
        row_accumulate<VEC, NT, G, U>(a.rowptr, a.col, a.eid, a.xj, a.dz, row, a.D, lig, gbase, acc);
        out = a.dxi;
    } else {
        if (!a.dxj) return;
        row_accumulate<VEC, NT, G, U>(a.rowptr_t, a.col_t, a.eid_t, a.xi, a.dz, row, a.D, lig, gbase, acc);
        out = a.dxj;
    }
#pragma unroll
    for (int tl = 0; tl < NT; ++tl) {
        const int f = (tl * G + lig) * VEC;
        if (f < a.D) Vec<VEC>::store(out + (int64_t)row * a.D + f, acc[tl]);
    }
}

}  // namespace
}  // namespace gnnmp

using namespace gnnmp;

extern "C" {

int gnnmp_negative_sample(const void *s, const void *t, int idx_bytes, int index_base, int64_t n_edges, int64_t n_nodes,
                          int64_t num_neg_edges, int bidirected, int max_trials, uint64_t seed, void *s_out, void *t_out,
                          int64_t capacity, int64_t *total, gnnmp_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (idx_bytes != 4 && idx_bytes != 8) return fail(GNNMP_EINVAL, "negative_sample: idx_bytes %d", idx_bytes);
    if (index_base != 0 && index_base != 1) return fail(GNNMP_EINVAL, "negative_sample: index_base %d", index_base);
    if (!total) return fail(GNNMP_EINVAL, "negative_sample: null total");
    *total = 0;
    if (n_edges < 0 || n_nodes < 0 || capacity < 0 || max_trials < 0) return fail(GNNMP_EINVAL, "negative_sample: negative size");
    if (num_neg_edges < 0) return fail(GNNMP_EINVAL, "negative_sample: num_neg_edges = %lld < 0", (long long)num_neg_edges);
    if (n_nodes > 0x7fffffffLL) return fail(GNNMP_EUNSUPPORTED, "negative_sample: more than 2^31 - 1 nodes");
    const int64_t num_neg = bidirected ? num_neg_edges / 2 : num_neg_edges;
    const uint64_t n = (uint64_t)n_nodes, maxid = n * n;
    // transform.jl:906-912 in Float64: the positives are g's edges plus a self loop on every node
    const double dmax = (double)maxid;
    const double pneg = 1.0 - (double)(n_edges + n_nodes) / (2.0 * dmax);
    double p = pneg == 0.0 ? 1.0 : std::min(1.0, (double)num_neg / (pneg * dmax) * 1.1);
    if (maxid == 0) p = 0.0;   // no codes to draw from (the reference's 0 / 0)
    if (p < 0.0 || std::isnan(p))
        return fail(GNNMP_EINVAL, "negative_sample: sample probability %g < 0 (%lld edges on %lld nodes)", p, (long long)n_edges,
                    (long long)n_nodes);
    const int64_t need = bidirected ? 2 * num_neg : num_neg;
    if (capacity < need) return fail(GNNMP_EINVAL, "negative_sample: capacity %lld < %lld", (long long)capacity, (long long)need);
    if (num_neg == 0 || p == 0.0 || max_trials == 0) return GNNMP_OK;
    if (!s_out || !t_out || (n_edges > 0 && (!s || !t))) return fail(GNNMP_EINVAL, "negative_sample: null pointer");

    const int code_bits = bit_length(maxid - 1);
    // chunks of about 32 expected candidates: enough threads, short walks
    const double expect = p * dmax;
    const uint64_t n_chunks = (uint64_t)std::min<double>(std::max(1.0, std::ceil(expect / 32.0)), (double)std::min<uint64_t>(maxid, 1ULL << 24));
    const uint64_t chunk_len = (maxid + n_chunks - 1) / n_chunks;
    const int64_t C = (int64_t)((maxid + chunk_len - 1) / chunk_len);
    const size_t scan_ws = exclusive_scan_workspace((size_t)(C + 1));
    // Destroyed in reverse order — codes_in, pos, kept, prev, counts, bad — when the call returns: the first hipFree waits for the
    // decode kernel, so the outputs are complete when the call returns.
    DevBuf<int> bad;
    DevBuf<int64_t> counts_buf;
    DevBuf<uint64_t> prev, kept, pos, codes_in;
    GNNMP_HIP(kept.alloc((size_t)num_neg));
    GNNMP_HIP(counts_buf.alloc(2 * (size_t)(C + 1) + scan_ws));
    GNNMP_HIP(bad.alloc(1));
    GNNMP_HIP(hipMemsetAsync(bad.get(), 0, sizeof(int), stream));
    int64_t *const counts = counts_buf.get();
    int hbad = 0;
    if (n_edges > 0) {
        GNNMP_HIP(codes_in.alloc((size_t)n_edges));
        GNNMP_HIP(pos.alloc((size_t)n_edges));
        edge_codes_kernel<<<nblk(n_edges), 256, 0, stream>>>(s, t, idx_bytes, index_base, n_edges, n_nodes, codes_in.get(), bad.get());
        GNNMP_HIP(hipGetLastError());
        // (synchronises the stream)
        GNNMP_TRY(radix_sort_keys_u64(codes_in.get(), pos.get(), (size_t)n_edges, 0, std::max(code_bits, 1), stream));
        GNNMP_HIP(hipMemcpyAsync(&hbad, bad.get(), sizeof(int), hipMemcpyDeviceToHost, stream));
    }
    NegTrialArgs a;
    a.pos = pos.get();
    a.n_pos = n_edges;
    a.prev = nullptr;
    a.n_prev = 0;
    a.maxid = maxid;
    a.chunk_len = chunk_len;
    a.n1 = n + 1;
    a.n_chunks = C;
    a.p_one = p >= 1.0;
    a.log1m_p = a.p_one ? -1.0 : std::log1p(-p);
    a.counts = counts;
    a.offsets = counts + (C + 1);
    int64_t *scan_scratch = counts + 2 * (C + 1);
    int64_t n_kept = 0;
    for (int trial = 0; trial < max_trials; ++trial) {
        // this trial's stream: independent of the chunking's other trials
        uint64_t z = seed + 0x9e3779b97f4a7c15ULL * (uint64_t)(trial + 1);
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
        z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
        a.stream = z ^ (z >> 31);
        a.out = kept.get() + n_kept;
        a.room = num_neg - n_kept;
        GNNMP_HIP(hipMemsetAsync(counts + C, 0, sizeof(int64_t), stream));
        neg_trial_kernel<0><<<nblk(C), 256, 0, stream>>>(a);
        GNNMP_HIP(hipGetLastError());
        GNNMP_TRY(exclusive_scan_i64(counts, counts + (C + 1), (size_t)(C + 1), stream, scan_scratch));
        int64_t got = 0;
        GNNMP_HIP(hipMemcpyAsync(&got, counts + (C + 1) + C, sizeof(int64_t), hipMemcpyDeviceToHost, stream));
        GNNMP_HIP(hipStreamSynchronize(stream));   // the one read of a trial
        if (hbad) return fail(GNNMP_EBOUNDS, "negative_sample: an edge index is outside the %lld nodes", (long long)n_nodes);
        if (got > 0) {
            neg_trial_kernel<1><<<nblk(C), 256, 0, stream>>>(a);
            GNNMP_HIP(hipGetLastError());
        }
        n_kept += std::min(got, a.room);
        if (n_kept >= num_neg || trial + 1 == max_trials) break;
        if (got > 0) {
            // the next trial looks codes up in everything kept so far, sorted (synchronises the stream)
            if (!prev.get()) GNNMP_HIP(prev.alloc((size_t)num_neg));
            GNNMP_TRY(radix_sort_keys_u64(kept.get(), prev.get(), (size_t)n_kept, 0, std::max(code_bits, 1), stream));
            a.prev = prev.get();
            a.n_prev = n_kept;
        }
    }
    if (n_kept > 0) {
        neg_decode_kernel<<<nblk(n_kept), 256, 0, stream>>>(kept.get(), n_kept, n, bidirected ? 1 : 0, idx_bytes, index_base, s_out, t_out);
        GNNMP_HIP(hipGetLastError());
    }
    *total = bidirected ? 2 * n_kept : n_kept;
    return GNNMP_OK;
}

int gnnmp_rand_edge_split(const void *s, const void *t, int idx_bytes, int index_base, int64_t n_edges, int bidirected, int64_t size1,
                          uint64_t seed, void *s1, void *t1, void *s2, void *t2, gnnmp_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (idx_bytes != 4 && idx_bytes != 8) return fail(GNNMP_EINVAL, "rand_edge_split: idx_bytes %d", idx_bytes);
    if (index_base != 0 && index_base != 1) return fail(GNNMP_EINVAL, "rand_edge_split: index_base %d", index_base);
    if (n_edges < 0) return fail(GNNMP_EINVAL, "rand_edge_split: negative size");
    const int64_t ne = bidirected ? n_edges / 2 : n_edges;
    if (size1 < 0 || size1 > ne) return fail(GNNMP_EINVAL, "rand_edge_split: size1 = %lld outside 0..%lld", (long long)size1, (long long)ne);
    if (ne == 0) return GNNMP_OK;
    if (!s || !t || (size1 > 0 && (!s1 || !t1)) || (size1 < ne && (!s2 || !t2)))
        return fail(GNNMP_EINVAL, "rand_edge_split: null pointer");
    const int ibits = std::max(1, bit_length((uint64_t)(ne - 1)));
    // (destroyed in reverse order — flags, kept, keys, sorted — when the call returns; the first hipFree waits for split_write_kernel)
    DevBuf<uint64_t> sorted, keys;
    DevBuf<int64_t> kept, flags_buf;
    if (bidirected) {
        // s .< t, compacted in edge order (transform.jl:959-960); the split draws from its first ne entries
        const size_t ws = exclusive_scan_workspace((size_t)(n_edges + 1));
        GNNMP_HIP(flags_buf.alloc(2 * (size_t)(n_edges + 1) + ws));
        GNNMP_HIP(kept.alloc((size_t)ne));
        int64_t *const flags = flags_buf.get();
        less_flag_kernel<<<nblk(n_edges + 1), 256, 0, stream>>>(s, t, idx_bytes, n_edges, flags);
        GNNMP_HIP(hipGetLastError());
        int64_t *posk = flags + (n_edges + 1);
        GNNMP_TRY(exclusive_scan_i64(flags, posk, (size_t)(n_edges + 1), stream, flags + 2 * (n_edges + 1)));
        int64_t m = 0;
        GNNMP_HIP(hipMemcpyAsync(&m, posk + n_edges, sizeof(int64_t), hipMemcpyDeviceToHost, stream));
        GNNMP_HIP(hipStreamSynchronize(stream));
        if (m < ne)
            return fail(GNNMP_EBOUNDS, "rand_edge_split(bidirected = true): %lld edges have s < t, fewer than num_edges / 2 = %lld "
                        "(the graph is not bidirected, or has self loops or multi-edges)", (long long)m, (long long)ne);
        less_compact_kernel<<<nblk(n_edges), 256, 0, stream>>>(flags, posk, n_edges, ne, kept.get());
        GNNMP_HIP(hipGetLastError());
    }
    GNNMP_HIP(keys.alloc((size_t)ne));
    GNNMP_HIP(sorted.alloc((size_t)ne));
    perm_keys_kernel<<<nblk(ne), 256, 0, stream>>>(ne, ibits, seed, keys.get());
    GNNMP_HIP(hipGetLastError());
    // randperm(ne) (synchronises the stream)
    GNNMP_TRY(radix_sort_keys_u64(keys.get(), sorted.get(), (size_t)ne, 0, 64, stream));
    split_write_kernel<<<nblk(ne), 256, 0, stream>>>(sorted.get(), ibits, kept.get(), s, t, idx_bytes, ne, size1, bidirected ? 1 : 0, s1, t1, s2,
                                                     t2);
    GNNMP_HIP(hipGetLastError());
    return GNNMP_OK;
}

int gnnmp_edge_dot_grad_f32(gnnmp_graph_t *plan, gnnmp_graph_t *plan_t, const float *xi, const float *xj, const float *dz, float *dxi,
                            float *dxj, int64_t D, gnnmp_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!plan || !plan_t) return fail(GNNMP_EINVAL, "edge_dot_grad: null plan");
    if (plan->self_loops || plan_t->self_loops) return fail(GNNMP_EINVAL, "edge_dot_grad: the plans must not add self loops");
    if (plan->n_dst != plan_t->n_dst || plan->n_src != plan->n_dst || plan->n_edges != plan_t->n_edges)
        return fail(GNNMP_EINVAL, "edge_dot_grad: the plans are not of one graph and its reverse");
    if (D <= 0) return fail(GNNMP_EINVAL, "edge_dot_grad: bad D");
    const bool alias = dxi == dxj;
    if (alias && xi != xj) return fail(GNNMP_EINVAL, "edge_dot_grad: one output (alias mode) needs xi == xj");
    if (!xi || !xj || (!dxi && !dxj) || (plan->n_edges > 0 && !dz)) return fail(GNNMP_EINVAL, "edge_dot_grad: null pointer");
    if (plan->n_dst == 0) return GNNMP_OK;
    uintptr_t m = reinterpret_cast<uintptr_t>(xi) | reinterpret_cast<uintptr_t>(xj) | reinterpret_cast<uintptr_t>(dxi) |
                  reinterpret_cast<uintptr_t>(dxj);
    int vec = pick_vec(D, reinterpret_cast<const void *>(m), reinterpret_cast<const void *>(m));
    const int64_t lanes = (D + vec - 1) / vec;
    if (D > 256) return fail(GNNMP_EUNSUPPORTED, "edge_dot_grad: D = %lld > 256; compose two propagates", (long long)D);
    int log2g = 0, nt = 1;
    while ((1LL << log2g) < lanes && log2g < 6) ++log2g;
    if (lanes > 64) nt = lanes > 128 ? 4 : 2;
    EdgeDotGradArgs a;
    a.rowptr = plan->rowptr;
    a.col = plan->col;
    a.eid = plan->eid;
    a.rowptr_t = plan_t->rowptr;
    a.col_t = plan_t->col;
    a.eid_t = plan_t->eid;
    a.xi = xi;
    a.xj = xj;
    a.dz = dz;
    a.dxi = dxi;
    a.dxj = dxj;
    a.alias = alias ? 1 : 0;
    a.D = (int)D;
    a.n_rows = (int)plan->n_dst;
    a.waves = 4;
    const int64_t rows = alias ? plan->n_dst : 2 * plan->n_dst;
    const int64_t rows_per_block = (int64_t)(64 >> log2g) * a.waves;
    const unsigned nb = (unsigned)((rows + rows_per_block - 1) / rows_per_block);
    with_vec(vec, [&](auto V) {
        constexpr int VEC = decltype(V)::value;
        if (nt == 4)
            edge_dot_grad_kernel<VEC, 6, 4><<<nb, 256, 0, stream>>>(a);
        else if (nt == 2)
            edge_dot_grad_kernel<VEC, 6, 2><<<nb, 256, 0, stream>>>(a);
        else
            with_log2g(log2g, [&](auto LG) { edge_dot_grad_kernel<VEC, decltype(LG)::value, 1><<<nb, 256, 0, stream>>>(a); });
    });
    GNNMP_LAUNCH_CHECK("edge_dot_grad_kernel");
    return GNNMP_OK;
}

}  // extern "C"
