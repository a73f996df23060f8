// coalesce.hip — the transforms that clean up the edge list itself, on the device:
//   remove_multi_edges(g; aggr)   GNNGraphs/src/transform.jl:157-185   gnnmp_coalesce_edges, DIRECTED
//   to_bidirected(g)              GNNGraphs/src/transform.jl:495-509   gnnmp_coalesce_edges, MIRRORED
//   to_unidirected(g)             GNNGraphs/src/transform.jl:517-529   gnnmp_coalesce_edges, UNDIRECTED
//   remove_self_loops(g)          GNNGraphs/src/transform.jl:49-64     gnnmp_compact_edges, SELF_LOOPS
//   remove_edges(g, idx | p)      GNNGraphs/src/transform.jl:121-146   gnnmp_compact_edges, LIST | RANDOM
//   has_multi_edges(g)            GNNGraphs/src/query.jl:575-579
//   has_isolated_nodes(g; dir)    GNNGraphs/src/query.jl:420-422
// The reference runs all of them on the CPU.  Integer work only — no float, no atomics on data: bit-exact by construction.
//
// Coalescing is a bipartite plan from input edges to output edges: the virtual edge positions are sorted STABLY by their packed
// (first, second) pair (sort_scan.hip's pair sort: element order inside a tile and tile order inside a digit are both kept, so equal
// keys stay in position order, like the reference's sortperm), a key larger than its predecessor starts an output edge, and the sorted
// positions ARE the plan's slots: colptr = the first slot of every output edge, rowval = the original row behind every slot.  The edge
// data is then reduced by the row kernel (propagate(copy_xj, aggr) over gnnmp_plan_from_csc of the two arrays), which adds in slot order.
#include <algorithm>

#include "common.h"
#include "scratch.h"
#include "sort_scan.h"

namespace gnnmp {
namespace {

inline unsigned nblk(int64_t n, int bs = 256) { return (unsigned)((n + bs - 1) / bs); }

// key of virtual position p: (first << 32) | second, both 0-based.  MIRRORED: position p >= E is edge p - E reversed (the second half
// of [s; t], [t; s]); UNDIRECTED: (min, max).  bad[0] = 1 for an index outside 0 .. n_nodes - 1 (n_nodes <= 2^32: a valid index fits
// 32 bits).  pos (nullable): the payload of the pair sort, pos[p] = p.
__global__ void coalesce_keys_kernel(const void *s, const void *t, int idx_bytes, int base, int64_t E, int64_t Ev, int64_t n_nodes,
                                     int mode, uint64_t *keys, uint32_t *pos, int *bad) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= Ev) return;
    const bool mirrored = p >= E;
    const int64_t k = mirrored ? p - E : p;
    const int64_t u = load_index(s, k, idx_bytes, base), v = load_index(t, k, idx_bytes, base);
    if (pos) pos[p] = (uint32_t)p;
    if (u < 0 || v < 0 || u >= n_nodes || v >= n_nodes) {
        *bad = 1;
        keys[p] = 0;
        return;
    }
    int64_t a = u, b = v;
    if (mode == GNNMP_COALESCE_UNDIRECTED) {
        a = min(u, v);
        b = max(u, v);
    } else if (mirrored) {
        a = v;
        b = u;
    }
    keys[p] = ((uint64_t)a << 32) | (uint64_t)b;
}

// head[i] = 1 where sorted slot i starts an output edge (idxs[2:end] .> idxs[1:end-1] with the -1 sentinel, transform.jl:169-170);
// head[Ev] = 0, so that the exclusive scan's last entry is the number of output edges
__global__ void coalesce_heads_kernel(const uint64_t *keys, int64_t Ev, uint32_t *head) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > Ev) return;
    head[i] = (i < Ev && (i == 0 || keys[i] != keys[i - 1])) ? 1u : 0u;
}

// the compaction: head slot i is output edge slot[i] — its endpoints from the key, its first sorted slot into colptr; the thread
// behind the last slot closes colptr with Ev
__global__ void coalesce_write_kernel(const uint64_t *keys, const uint32_t *head, const uint32_t *slot, int64_t Ev, int idx_bytes,
                                      int base, void *s_out, void *t_out, void *colptr) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > Ev) return;
    if (i == Ev) {
        store_index(colptr, (int64_t)slot[Ev], idx_bytes, Ev + base);
        return;
    }
    if (!head[i]) return;
    const int64_t o = (int64_t)slot[i];
    store_index(s_out, o, idx_bytes, (int64_t)(keys[i] >> 32) + base);
    store_index(t_out, o, idx_bytes, (int64_t)(keys[i] & 0xffffffffULL) + base);
    store_index(colptr, o, idx_bytes, i + base);
}

// rowval[i] = the row of the original edge data behind sorted slot i: a virtual position p >= E reads row p - E
__global__ void coalesce_fold_kernel(const uint32_t *pos, int64_t E, int64_t Ev, int idx_bytes, int base, void *rowval) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Ev) return;
    const int64_t p = (int64_t)pos[i];
    store_index(rowval, i, idx_bytes, (p >= E ? p - E : p) + base);
}

__global__ void equal_neighbours_kernel(const uint64_t *keys, int64_t E, int *flag) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i + 1 < E && keys[i] == keys[i + 1]) *flag = 1;
}

__global__ void empty_row_kernel(const uint32_t *rowptr, int64_t n_rows, int *flag) {
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v < n_rows && rowptr[v] == rowptr[v + 1]) *flag = 1;
}

// ---- stream compaction -----------------------------------------------------------------------------------------------------
struct CompactArgs {
    const void *s, *t;
    const float *w;
    int idx_bytes, base;
    int64_t E;
    int rule;
    uint32_t thr, seed_lo, seed_hi;   // RANDOM: kept when drop_bits(seed, e, 0) >= thr (common.h); none: p = 1
    int none;
    uint32_t *keep;                   // [E + 1], keep[E] = 0
    const uint32_t *slot;             // exclusive scan of keep
    const int *bad;
    void *s_out, *t_out, *eid_out;
    float *w_out;
};

__global__ void compact_keep_kernel(const CompactArgs a) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k > a.E) return;
    uint32_t keep = 0;
    if (k < a.E) {
        if (a.rule == GNNMP_COMPACT_SELF_LOOPS)
            keep = load_index(a.s, k, a.idx_bytes, 0) != load_index(a.t, k, a.idx_bytes, 0);
        else if (a.rule == GNNMP_COMPACT_LIST)
            keep = 1;   // compact_mark_kernel clears the listed positions
        else
            keep = !a.none && drop_bits(a.seed_lo, a.seed_hi, (uint32_t)k, 0u) >= a.thr;
    }
    a.keep[k] = keep;
}

// keep[remove[j]] = 0 (every writer of a word stores the same value: repeats are harmless); bad[0] = 1 for a position outside 0 .. E - 1
__global__ void compact_mark_kernel(const void *remove, int idx_bytes, int base, int64_t n_remove, int64_t E, uint32_t *keep, int *bad) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_remove) return;
    const int64_t k = load_index(remove, j, idx_bytes, base);
    if (k < 0 || k >= E) {
        *bad = 1;
        return;
    }
    keep[k] = 0;
}

// kept edge k goes to slot[k]: raw index values (width and base kept), its weight, and its own position as eid.  Writes nothing when
// the list held a bad position.
__global__ void compact_write_kernel(const CompactArgs a) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= a.E || *a.bad || !a.keep[k]) return;
    const int64_t o = (int64_t)a.slot[k];
    store_index(a.s_out, o, a.idx_bytes, load_index(a.s, k, a.idx_bytes, 0));
    store_index(a.t_out, o, a.idx_bytes, load_index(a.t, k, a.idx_bytes, 0));
    store_index(a.eid_out, o, a.idx_bytes, k + a.base);
    if (a.w_out) a.w_out[o] = a.w[k];
}

constexpr int64_t TWO32 = (int64_t)1 << 32;

}  // namespace
}  // namespace gnnmp

using namespace gnnmp;

extern "C" {

int gnnmp_coalesce_edges(const gnnmp_coalesce_t *job, int64_t *total, gnnmp_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!job) return fail(GNNMP_EINVAL, "coalesce_edges: null job");
    if (!total) return fail(GNNMP_EINVAL, "coalesce_edges: null total");
    *total = 0;
    const int idx_bytes = job->idx_bytes, base = job->index_base, mode = job->mode;
    const int64_t E = job->n_edges, n_nodes = job->n_nodes;
    if (idx_bytes != 4 && idx_bytes != 8) return fail(GNNMP_EINVAL, "coalesce_edges: idx_bytes %d", idx_bytes);
    if (base != 0 && base != 1) return fail(GNNMP_EINVAL, "coalesce_edges: index_base %d", base);
    if (mode != GNNMP_COALESCE_DIRECTED && mode != GNNMP_COALESCE_MIRRORED && mode != GNNMP_COALESCE_UNDIRECTED)
        return fail(GNNMP_EINVAL, "coalesce_edges: mode %d", mode);
    if (E < 0 || n_nodes < 0) return fail(GNNMP_EINVAL, "coalesce_edges: negative size");
    if (E == 0) return GNNMP_OK;
    if (!job->s || !job->t || !job->s_out || !job->t_out || !job->colptr || !job->rowval)
        return fail(GNNMP_EINVAL, "coalesce_edges: null pointer");
    if (n_nodes > TWO32) return fail(GNNMP_EBOUNDS, "coalesce_edges: %lld nodes: indices must fit 32 bits", (long long)n_nodes);
    if (E >= TWO32 || (mode == GNNMP_COALESCE_MIRRORED ? 2 * E : E) >= TWO32)
        return fail(GNNMP_EBOUNDS, "coalesce_edges: %lld edge positions do not fit the pair sort's 32-bit values",
                    (long long)(mode == GNNMP_COALESCE_MIRRORED ? 2 * E : E));
    const int64_t Ev = mode == GNNMP_COALESCE_MIRRORED ? 2 * E : E;
    if (idx_bytes == 4 && Ev + base > 0x7fffffffLL)
        return fail(GNNMP_EBOUNDS, "coalesce_edges: colptr values up to %lld do not fit the 4-byte index type", (long long)(Ev + base));

    // (destroyed in reverse order when the call returns; the stream is synchronised behind the last kernel before that)
    DevBuf<int> bad;
    DevBuf<uint32_t> heads, pos_sorted, pos_in;
    DevBuf<uint64_t> keys_sorted, keys_in;
    GNNMP_HIP(keys_in.alloc((size_t)Ev));
    GNNMP_HIP(keys_sorted.alloc((size_t)Ev));
    GNNMP_HIP(pos_in.alloc((size_t)Ev));
    GNNMP_HIP(pos_sorted.alloc((size_t)Ev));
    GNNMP_HIP(heads.alloc(2 * (size_t)(Ev + 1) + exclusive_scan_workspace((size_t)(Ev + 1))));
    GNNMP_HIP(bad.alloc(1));
    GNNMP_HIP(hipMemsetAsync(bad.get(), 0, sizeof(int), stream));
    coalesce_keys_kernel<<<nblk(Ev), 256, 0, stream>>>(job->s, job->t, idx_bytes, base, E, Ev, n_nodes, mode, keys_in.get(), pos_in.get(),
                                                        bad.get());
    GNNMP_HIP(hipGetLastError());
    // (synchronises the stream)
    GNNMP_TRY(radix_sort_pairs_u64(keys_in.get(), keys_sorted.get(), pos_in.get(), pos_sorted.get(), (size_t)Ev, 0, 64, stream));
    int hbad = 0;
    GNNMP_HIP(hipMemcpyAsync(&hbad, bad.get(), sizeof(int), hipMemcpyDeviceToHost, stream));
    GNNMP_HIP(hipStreamSynchronize(stream));
    if (hbad) return fail(GNNMP_EBOUNDS, "coalesce_edges: an edge index is outside the %lld nodes", (long long)n_nodes);

    uint32_t *const head = heads.get(), *const slot = head + (Ev + 1), *const scan_ws = head + 2 * (Ev + 1);
    coalesce_heads_kernel<<<nblk(Ev + 1), 256, 0, stream>>>(keys_sorted.get(), Ev, head);
    GNNMP_HIP(hipGetLastError());
    GNNMP_TRY(exclusive_scan_u32(head, slot, (size_t)(Ev + 1), stream, scan_ws));
    coalesce_write_kernel<<<nblk(Ev + 1), 256, 0, stream>>>(keys_sorted.get(), head, slot, Ev, idx_bytes, base, job->s_out, job->t_out,
                                                            job->colptr);
    GNNMP_HIP(hipGetLastError());
    coalesce_fold_kernel<<<nblk(Ev), 256, 0, stream>>>(pos_sorted.get(), E, Ev, idx_bytes, base, job->rowval);
    GNNMP_HIP(hipGetLastError());
    uint32_t tot = 0;
    GNNMP_HIP(hipMemcpyAsync(&tot, slot + Ev, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    GNNMP_HIP(hipStreamSynchronize(stream));
    *total = (int64_t)tot;
    return GNNMP_OK;
}

int gnnmp_compact_edges(const gnnmp_compact_t *job, int64_t *total, gnnmp_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!job) return fail(GNNMP_EINVAL, "compact_edges: null job");
    if (!total) return fail(GNNMP_EINVAL, "compact_edges: null total");
    *total = 0;
    const int idx_bytes = job->idx_bytes, base = job->index_base, rule = job->rule;
    const int64_t E = job->n_edges;
    if (idx_bytes != 4 && idx_bytes != 8) return fail(GNNMP_EINVAL, "compact_edges: idx_bytes %d", idx_bytes);
    if (base != 0 && base != 1) return fail(GNNMP_EINVAL, "compact_edges: index_base %d", base);
    if (rule != GNNMP_COMPACT_SELF_LOOPS && rule != GNNMP_COMPACT_LIST && rule != GNNMP_COMPACT_RANDOM)
        return fail(GNNMP_EINVAL, "compact_edges: rule %d", rule);
    if (E < 0) return fail(GNNMP_EINVAL, "compact_edges: negative size");
    if (rule == GNNMP_COMPACT_LIST && job->n_remove < 0) return fail(GNNMP_EINVAL, "compact_edges: negative n_remove");
    if (rule == GNNMP_COMPACT_RANDOM && !(job->p >= 0.0f && job->p <= 1.0f))
        return fail(GNNMP_EINVAL, "compact_edges: probability %g outside [0, 1]", (double)job->p);
    if ((job->w == nullptr) != (job->w_out == nullptr)) return fail(GNNMP_EINVAL, "compact_edges: w and w_out go together");
    if (E == 0) return GNNMP_OK;
    if (!job->s || !job->t || !job->s_out || !job->t_out || !job->eid_out) return fail(GNNMP_EINVAL, "compact_edges: null pointer");
    const int64_t n_remove = rule == GNNMP_COMPACT_LIST ? job->n_remove : 0;
    if (n_remove > 0 && !job->remove) return fail(GNNMP_EINVAL, "compact_edges: null remove list");
    if (E >= TWO32) return fail(GNNMP_EBOUNDS, "compact_edges: %lld edge positions do not fit 32 bits", (long long)E);
    if (idx_bytes == 4 && E - 1 + base > 0x7fffffffLL)
        return fail(GNNMP_EBOUNDS, "compact_edges: edge positions up to %lld do not fit the 4-byte index type", (long long)(E - 1 + base));

    DevBuf<int> bad;
    DevBuf<uint32_t> keep;
    GNNMP_HIP(keep.alloc(2 * (size_t)(E + 1) + exclusive_scan_workspace((size_t)(E + 1))));
    GNNMP_HIP(bad.alloc(1));
    GNNMP_HIP(hipMemsetAsync(bad.get(), 0, sizeof(int), stream));
    CompactArgs a;
    a.s = job->s;
    a.t = job->t;
    a.w = job->w;
    a.idx_bytes = idx_bytes;
    a.base = base;
    a.E = E;
    a.rule = rule;
    const DropArgs d = make_drop(rule == GNNMP_COMPACT_RANDOM && job->p < 1.0f ? job->p : 0.0f, job->seed);
    a.thr = d.thr;
    a.seed_lo = d.seed_lo;
    a.seed_hi = d.seed_hi;
    a.none = rule == GNNMP_COMPACT_RANDOM && job->p >= 1.0f;
    a.keep = keep.get();
    a.slot = keep.get() + (E + 1);
    a.bad = bad.get();
    a.s_out = job->s_out;
    a.t_out = job->t_out;
    a.eid_out = job->eid_out;
    a.w_out = job->w_out;
    compact_keep_kernel<<<nblk(E + 1), 256, 0, stream>>>(a);
    GNNMP_HIP(hipGetLastError());
    if (n_remove > 0) {
        compact_mark_kernel<<<nblk(n_remove), 256, 0, stream>>>(job->remove, idx_bytes, base, n_remove, E, keep.get(), bad.get());
        GNNMP_HIP(hipGetLastError());
    }
    GNNMP_TRY(exclusive_scan_u32(keep.get(), keep.get() + (E + 1), (size_t)(E + 1), stream, keep.get() + 2 * (E + 1)));
    compact_write_kernel<<<nblk(E), 256, 0, stream>>>(a);
    GNNMP_HIP(hipGetLastError());
    int hbad = 0;
    uint32_t tot = 0;
    GNNMP_HIP(hipMemcpyAsync(&tot, a.slot + E, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    GNNMP_HIP(hipMemcpyAsync(&hbad, bad.get(), sizeof(int), hipMemcpyDeviceToHost, stream));
    GNNMP_HIP(hipStreamSynchronize(stream));
    if (hbad) return fail(GNNMP_EBOUNDS, "compact_edges: a listed position is outside the %lld edges", (long long)E);
    *total = (int64_t)tot;
    return GNNMP_OK;
}

int gnnmp_has_multi_edges(const void *s, const void *t, int idx_bytes, int index_base, int64_t n_edges, int *result,
                          gnnmp_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (idx_bytes != 4 && idx_bytes != 8) return fail(GNNMP_EINVAL, "has_multi_edges: idx_bytes %d", idx_bytes);
    if (index_base != 0 && index_base != 1) return fail(GNNMP_EINVAL, "has_multi_edges: index_base %d", index_base);
    if (!result) return fail(GNNMP_EINVAL, "has_multi_edges: null result");
    *result = 0;
    if (n_edges <= 0) return n_edges < 0 ? fail(GNNMP_EINVAL, "has_multi_edges: negative size") : GNNMP_OK;
    if (!s || !t) return fail(GNNMP_EINVAL, "has_multi_edges: null pointer");
    if (n_edges >= TWO32) return fail(GNNMP_EBOUNDS, "has_multi_edges: %lld edges exceed the sort's 32-bit offsets", (long long)n_edges);
    DevBuf<int> flags;   // [0] an index that does not fit 32 bits, [1] two equal neighbours
    DevBuf<uint64_t> keys_sorted, keys_in;
    GNNMP_HIP(keys_in.alloc((size_t)n_edges));
    GNNMP_HIP(keys_sorted.alloc((size_t)n_edges));
    GNNMP_HIP(flags.alloc(2));
    GNNMP_HIP(hipMemsetAsync(flags.get(), 0, 2 * sizeof(int), stream));
    coalesce_keys_kernel<<<nblk(n_edges), 256, 0, stream>>>(s, t, idx_bytes, index_base, n_edges, n_edges, TWO32, GNNMP_COALESCE_DIRECTED,
                                                            keys_in.get(), nullptr, flags.get());
    GNNMP_HIP(hipGetLastError());
    // (synchronises the stream)
    GNNMP_TRY(radix_sort_keys_u64(keys_in.get(), keys_sorted.get(), (size_t)n_edges, 0, 64, stream));
    equal_neighbours_kernel<<<nblk(n_edges), 256, 0, stream>>>(keys_sorted.get(), n_edges, flags.get() + 1);
    GNNMP_HIP(hipGetLastError());
    int h[2] = {0, 0};
    GNNMP_HIP(hipMemcpyAsync(h, flags.get(), 2 * sizeof(int), hipMemcpyDeviceToHost, stream));
    GNNMP_HIP(hipStreamSynchronize(stream));
    if (h[0]) return fail(GNNMP_EBOUNDS, "has_multi_edges: an index is negative or does not fit 32 bits");
    *result = h[1] ? 1 : 0;
    return GNNMP_OK;
}

int gnnmp_has_isolated_nodes(gnnmp_graph_t *plan, int *result, gnnmp_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!plan) return fail(GNNMP_EINVAL, "has_isolated_nodes: null plan");
    if (!result) return fail(GNNMP_EINVAL, "has_isolated_nodes: null result");
    *result = 0;
    if (plan->n_dst == 0) return GNNMP_OK;
    DevBuf<int> flag;
    GNNMP_HIP(flag.alloc(1));
    GNNMP_HIP(hipMemsetAsync(flag.get(), 0, sizeof(int), stream));
    empty_row_kernel<<<nblk(plan->n_dst), 256, 0, stream>>>(plan->rowptr, plan->n_dst, flag.get());
    GNNMP_HIP(hipGetLastError());
    int h = 0;
    GNNMP_HIP(hipMemcpyAsync(&h, flag.get(), sizeof(int), hipMemcpyDeviceToHost, stream));
    GNNMP_HIP(hipStreamSynchronize(stream));
    *result = h ? 1 : 0;
    return GNNMP_OK;
}

}  // extern "C"
