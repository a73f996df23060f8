// plan_edit.hip — the plan of an EDITED graph from the plan of its parent, without a sort of the parent's edges.
//   remove_nodes (GNNGraphs/src/transform.jl:212-276), add_edges (:319-353), add_nodes and perturb_edges (:385-420) are the augmentations
//   of contrastive / robust training: applied to a fresh batch on every step and convolved at once, so the child's PLAN is per-step work.
//   The child's dst-sorted stable CSR is a filtered, relabelled copy of the parent's:
//     gnnmp_plan_remove_nodes   the surviving slots of the surviving rows, in the parent's order — the child's slot array is the parent's
//                               with the dead slots squeezed out, so ONE exclusive scan over the per-slot keep flags gives every slot its
//                               place and every row its rowptr (rowptr'[new(i)] = scan[rowptr[i]]); two more scans renumber nodes and edges
//     gnnmp_plan_add_edges      every row is the parent's row followed by its new slots in position order (a plan-added self loop stays
//                               last): the m NEW edges are grouped by destination with the stable radix sort (sort_scan.h), the parent's
//                               E edges only shift by the new slots before them
//   Integer work only: flags, scans, copies; atomics only for a maximum (the child's longest row) and the bad-index flag.  The plan's arrays
//   come from the stream-ordered pool like gnnmp_plan_select's (plan_batch.hip: pooled_plan_alloc), and so does the scratch, which goes
//   back to the pool behind the last kernel that reads it — no hipFree, no wait.
#include <algorithm>

#include "common.h"
#include "launch.h"
#include "pool.h"
#include "sort_scan.h"

namespace gnnmp {
namespace {

constexpr int BS = 256;
inline unsigned nblk(int64_t n) { return (unsigned)std::max<int64_t>(1, (n + BS - 1) / BS); }
inline size_t up64(size_t n) { return (n + 63) & ~(size_t)63; }   // (pieces of the scratch block start on 256-byte boundaries)

// a block of the pool for the length of one call: parked again, behind the work enqueued on `stream`, when the call returns
struct PoolScratch {
    void *p = nullptr;
    size_t cap = 0;
    hipStream_t stream;
    explicit PoolScratch(hipStream_t s) : stream(s) {}
    PoolScratch(const PoolScratch &) = delete;
    PoolScratch &operator=(const PoolScratch &) = delete;
    ~PoolScratch() { pool_park(p, cap, stream, true); }
    bool take(size_t bytes) { return pool_take(&p, &cap, std::max<size_t>(bytes, 256), stream); }
};

// the row of slot p < rowptr[n_rows]: the largest i with rowptr[i] <= p
__device__ __forceinline__ int64_t row_of_slot(const uint32_t *__restrict__ rowptr, int64_t n_rows, int64_t p) {
    int64_t lo = 0, hi = n_rows;
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t)rowptr[mid] <= p) lo = mid; else hi = mid;
    }
    return lo;
}

// ==== remove_nodes =====================================================================================================================
// meta words of one call (zeroed before the first kernel)
enum { META_NKEEP = 0, META_EKEEP = 1, META_SLOTS = 2, META_MAXDEG = 3, META_BAD = 4, META_WORDS = 8 };

// keep[i] for i < N: 1 in list mode (the list clears its entries next), the mask of gnnmp_dropout_keep_u8(seed, p, N, 1) in random mode
// (`none`: p = 1, nothing kept); keep[N] = 0 closes the scan
__global__ void __launch_bounds__(BS) rm_mark_kernel(int64_t N, int random, int none, DropArgs d, uint32_t *__restrict__ keep) {
    const int64_t i = (int64_t)blockIdx.x * BS + threadIdx.x;
    if (i > N) return;
    uint32_t k = 0;
    if (i < N) k = !random ? 1u : (none ? 0u : (drop_bits(d.seed_lo, d.seed_hi, (uint32_t)i, 0u) >= d.thr ? 1u : 0u));
    keep[i] = k;
}
__global__ void __launch_bounds__(BS) rm_list_kernel(const void *__restrict__ remove, int idx_bytes, int base, int64_t n_remove, int64_t N,
                                                     uint32_t *__restrict__ keep, uint32_t *__restrict__ meta) {
    const int64_t j = (int64_t)blockIdx.x * BS + threadIdx.x;
    if (j >= n_remove) return;
    const int64_t k = load_index(remove, j, idx_bytes, base);
    if (k < 0 || k >= N) {
        meta[META_BAD] = 1;
        return;
    }
    keep[k] = 0;      // (repeats store the same value)
}
// keep[i] = (mask[i] != 0) for i < N, keep[N] = 0: the caller's mask in the 0 / 1 form the scans add up (gnnmp_plan_keep_nodes)
__global__ void __launch_bounds__(BS) rm_mask_kernel(int64_t N, const uint32_t *__restrict__ mask, uint32_t *__restrict__ keep) {
    const int64_t i = (int64_t)blockIdx.x * BS + threadIdx.x;
    if (i > N) return;
    keep[i] = i < N && mask[i] != 0u ? 1u : 0u;
}
// slot p of row i holds edge (col[p] -> i): it survives iff both ends do (a plan-added self loop has col = i).  Every original edge
// owns exactly one slot, so the loop over slots also writes the keep flag of every edge POSITION.  Thread T closes both scans.
__global__ void __launch_bounds__(BS) rm_slot_kernel(const uint32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                     const int32_t *__restrict__ eid, int64_t N, int64_t T, int64_t E,
                                                     const uint32_t *__restrict__ keep, uint32_t *__restrict__ skeep,
                                                     uint32_t *__restrict__ ekeep) {
    const int64_t p = (int64_t)blockIdx.x * BS + threadIdx.x;
    if (p > T) return;
    if (p == T) {
        skeep[T] = 0;
        ekeep[E] = 0;
        return;
    }
    const int64_t i = row_of_slot(rowptr, N, p);
    const uint32_t k = keep[i] & keep[col[p]];
    skeep[p] = k;
    const int64_t e = (uint32_t)eid[p];
    if (e < E) ekeep[e] = k;
}
// the totals the host needs, in one place: nodes, edges and slots kept, the child's longest row
__global__ void __launch_bounds__(BS) rm_meta_kernel(const uint32_t *__restrict__ rowptr, int64_t N, int64_t T, int64_t E,
                                                     const uint32_t *__restrict__ keep, const uint32_t *__restrict__ newid,
                                                     const uint32_t *__restrict__ spos, const uint32_t *__restrict__ erank,
                                                     uint32_t *__restrict__ meta) {
    const int64_t i = (int64_t)blockIdx.x * BS + threadIdx.x;
    if (i == 0) {
        meta[META_NKEEP] = newid[N];
        meta[META_EKEEP] = erank[E];
        meta[META_SLOTS] = spos[T];
    }
    uint32_t len = 0;
    if (i < N && keep[i]) len = spos[rowptr[i + 1]] - spos[rowptr[i]];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) len = max(len, (uint32_t)__shfl_xor((int)len, o, 64));
    if ((threadIdx.x & 63) == 0 && len > 0) atomicMax(meta + META_MAXDEG, len);
}
struct RmFill {
    const uint32_t *rowptr;
    const int32_t *col, *eid;
    int64_t N, T, E;
    const uint32_t *keep, *newid, *skeep, *spos, *ekeep, *erank;
    uint32_t n_keep, e_keep, n_slots;
    uint32_t *rowptr_out;
    int32_t *col_out, *eid_out;
    int32_t *node_map, *node_new;
    uint32_t *edge_map;
    unsigned row_blocks, slot_blocks;
};
// blocks [0, row_blocks): rowptr' and the node maps; the next slot_blocks: col' and eid'; the rest: the edge map
__global__ void __launch_bounds__(BS) rm_fill_kernel(const RmFill a) {
    if (blockIdx.x < a.row_blocks) {
        const int64_t i = (int64_t)blockIdx.x * BS + threadIdx.x;
        if (i > a.N) return;
        if (i == a.N) {
            a.rowptr_out[a.n_keep] = a.n_slots;
            return;
        }
        const uint32_t k = a.keep[i], nn = a.newid[i];
        if (a.node_new) a.node_new[i] = k ? (int32_t)nn : -1;
        if (!k) return;
        a.rowptr_out[nn] = a.spos[a.rowptr[i]];
        if (a.node_map) a.node_map[nn] = (int32_t)i;
    } else if (blockIdx.x < a.row_blocks + a.slot_blocks) {
        const int64_t p = (int64_t)(blockIdx.x - a.row_blocks) * BS + threadIdx.x;
        if (p >= a.T || !a.skeep[p]) return;
        const uint32_t q = a.spos[p];
        const uint32_t c = a.newid[a.col[p]];
        const int64_t e = (uint32_t)a.eid[p];
        a.col_out[q] = (int32_t)c;
        a.eid_out[q] = (int32_t)(e < a.E ? a.erank[e] : a.e_keep + c);      // (a plan-added self loop: col = its node)
    } else {
        const int64_t e = (int64_t)(blockIdx.x - a.row_blocks - a.slot_blocks) * BS + threadIdx.x;
        if (e >= a.E || !a.ekeep[e]) return;
        a.edge_map[a.erank[e]] = (uint32_t)e;
    }
}

// ==== add_edges ========================================================================================================================
__device__ __forceinline__ uint32_t mulhi32(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a * (uint64_t)b) >> 32); }

// keys[k] = 0-based destination of new edge k, vals[k] = k, snew[k] = its 0-based source.  List mode reads (and range-checks) the
// caller's pairs; random mode draws pair k from the dropout hash of (seed, k, 0 | 1) and writes it to the caller's outputs.
__global__ void __launch_bounds__(BS) ae_keys_kernel(const void *__restrict__ s_new, const void *__restrict__ t_new, int idx_bytes,
                                                     int base, int64_t m, int64_t N, int64_t n_nodes, uint32_t seed_lo, uint32_t seed_hi,
                                                     void *__restrict__ s_out, void *__restrict__ t_out, uint32_t *__restrict__ keys,
                                                     uint32_t *__restrict__ vals, int32_t *__restrict__ snew, uint32_t *__restrict__ bad) {
    const int64_t k = (int64_t)blockIdx.x * BS + threadIdx.x;
    if (k >= m) return;
    int64_t s, t;
    if (s_new) {
        s = load_index(s_new, k, idx_bytes, base);
        t = load_index(t_new, k, idx_bytes, base);
        if (s < 0 || s >= n_nodes || t < 0 || t >= n_nodes) {
            *bad = 1;
            s = t = 0;
        }
    } else {
        s = mulhi32(drop_bits(seed_lo, seed_hi, (uint32_t)k, 0u), (uint32_t)N);
        const uint32_t tp = mulhi32(drop_bits(seed_lo, seed_hi, (uint32_t)k, 1u), (uint32_t)(N - 1));
        t = (int64_t)tp + (tp >= (uint32_t)s ? 1 : 0);
        store_index(s_out, k, idx_bytes, s + base);
        store_index(t_out, k, idx_bytes, t + base);
    }
    keys[k] = (uint32_t)t;
    vals[k] = (uint32_t)k;
    snew[k] = (int32_t)s;
}
// newptr[i] = the number of new edges whose destination is below i (lower bound in the sorted keys), i = 0 .. n_nodes
__global__ void __launch_bounds__(BS) ae_newptr_kernel(const uint32_t *__restrict__ keys, int64_t m, int64_t n_nodes,
                                                       uint32_t *__restrict__ newptr) {
    const int64_t i = (int64_t)blockIdx.x * BS + threadIdx.x;
    if (i > n_nodes) return;
    int64_t lo = 0, hi = m;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t)keys[mid] < i) lo = mid + 1; else hi = mid;
    }
    newptr[i] = (uint32_t)lo;
}
struct AeFill {
    const uint32_t *rowptr;
    const int32_t *col, *eid;
    int64_t N, T, E, m, n_nodes;
    int loops;
    const uint32_t *keys, *vals, *newptr;     // the new edges sorted by destination
    const int32_t *snew;
    uint32_t *rowptr_out;
    int32_t *col_out, *eid_out;
    unsigned row_blocks, slot_blocks;
};
// slots before row i of the child: the parent's, the new edges into rows below i, the self loops of the new nodes below i
__device__ __forceinline__ uint32_t ae_row_begin(const AeFill &a, int64_t i) {
    return (i <= a.N ? a.rowptr[i] : (uint32_t)a.T) + a.newptr[i] + (a.loops && i > a.N ? (uint32_t)(i - a.N) : 0u);
}
// blocks [0, row_blocks): rowptr' and the self loops of the new nodes; the next slot_blocks: the parent's slots; the rest: the new edges
__global__ void __launch_bounds__(BS) ae_fill_kernel(const AeFill a) {
    const uint32_t e_child = (uint32_t)(a.E + a.m);
    if (blockIdx.x < a.row_blocks) {
        const int64_t i = (int64_t)blockIdx.x * BS + threadIdx.x;
        if (i > a.n_nodes) return;
        a.rowptr_out[i] = ae_row_begin(a, i);
        if (a.loops && i >= a.N && i < a.n_nodes) {
            const uint32_t q = ae_row_begin(a, i + 1) - 1;
            a.col_out[q] = (int32_t)i;
            a.eid_out[q] = (int32_t)(e_child + (uint32_t)i);
        }
    } else if (blockIdx.x < a.row_blocks + a.slot_blocks) {
        const int64_t p = (int64_t)(blockIdx.x - a.row_blocks) * BS + threadIdx.x;
        if (p >= a.T) return;
        const int64_t i = row_of_slot(a.rowptr, a.N, p);
        const int64_t e = (uint32_t)a.eid[p];
        const bool loop = e >= a.E;                                   // the row's last slot: it moves behind the row's new slots
        const uint32_t q = (uint32_t)p + a.newptr[loop ? i + 1 : i];
        a.col_out[q] = a.col[p];
        a.eid_out[q] = (int32_t)(loop ? e_child + (uint32_t)i : (uint32_t)e);
    } else {
        const int64_t j = (int64_t)(blockIdx.x - a.row_blocks - a.slot_blocks) * BS + threadIdx.x;
        if (j >= a.m) return;
        const int64_t d = a.keys[j];
        const uint32_t own = d < a.N ? a.rowptr[d + 1] - a.rowptr[d] - (a.loops ? 1u : 0u) : 0u;
        const uint32_t q = ae_row_begin(a, d) + own + ((uint32_t)j - a.newptr[d]);
        const uint32_t k = a.vals[j];
        a.col_out[q] = a.snew[k];
        a.eid_out[q] = (int32_t)((uint32_t)a.E + k);
    }
}

int check_common(const char *who, gnnmp_graph_t **out, const gnnmp_graph_t *parent, int idx_bytes, int index_base) {
    if (!out) return fail(GNNMP_EINVAL, "%s: out is NULL", who);
    *out = nullptr;
    if (!parent) return fail(GNNMP_EINVAL, "%s: parent is NULL", who);
    if (idx_bytes != 4 && idx_bytes != 8) return fail(GNNMP_EINVAL, "%s: idx_bytes must be 4 or 8 (got %d)", who, idx_bytes);
    if (index_base != 0 && index_base != 1) return fail(GNNMP_EINVAL, "%s: index_base must be 0 or 1 (got %d)", who, index_base);
    if (parent->n_src != parent->n_dst)
        return fail(GNNMP_EINVAL, "%s: the parent plan is not a square graph (%lld sources, %lld destinations)", who,
                    (long long)parent->n_src, (long long)parent->n_dst);
    return GNNMP_OK;
}

// how the keep flags of a call come about: the caller's mask (gnnmp_plan_keep_nodes), or a list / a Bernoulli draw (gnnmp_plan_remove_nodes)
struct RmMark {
    bool by_mask = false;
    const uint32_t *mask = nullptr;
    const void *remove = nullptr;
    int idx_bytes = 8, index_base = 0;
    int64_t n_remove = 0;
    float p = 0.0f;
    uint64_t seed = 0;
};

// the body the two exports share: everything after the argument checks — the mark, the three scans, the one synchronisation, the fill
int rm_derive(const char *who, gnnmp_graph_t **out, const gnnmp_graph_t *parent, const RmMark &m, int32_t *node_map_out,
              int32_t *node_new_out, uint32_t *edge_map_out, int64_t *total, hipStream_t stream) {
    const int64_t N = parent->n_dst, T = parent->n_total, E = parent->n_edges;
    const int loops = parent->self_loops;

    // scratch: keep | newid [N + 1], skeep | spos [T + 1], ekeep | erank [E + 1], the scans' block sums, the meta words
    const size_t nN = up64((size_t)N + 1), nT = up64((size_t)T + 1), nE = up64((size_t)E + 1);
    const size_t nW = up64(std::max(exclusive_scan_workspace((size_t)N + 1),
                                    std::max(exclusive_scan_workspace((size_t)T + 1), exclusive_scan_workspace((size_t)E + 1))));
    PoolScratch sc(stream);
    const size_t words = 2 * nN + 2 * nT + 2 * nE + nW + up64(META_WORDS);
    if (!sc.take(sizeof(uint32_t) * words)) return fail(GNNMP_EALLOC, "%s: hipMalloc of %zu bytes failed", who, 4 * words);
    uint32_t *const keep = static_cast<uint32_t *>(sc.p), *const newid = keep + nN, *const skeep = newid + nN, *const spos = skeep + nT,
                   *const ekeep = spos + nT, *const erank = ekeep + nE, *const scan_ws = erank + nE, *const meta = scan_ws + nW;
    GNNMP_HIP(hipMemsetAsync(meta, 0, sizeof(uint32_t) * META_WORDS, stream));

    if (m.by_mask) {
        rm_mask_kernel<<<nblk(N + 1), BS, 0, stream>>>(N, m.mask, keep);
        GNNMP_LAUNCH_CHECK("rm_mask_kernel");
    } else {
        const bool random = m.remove == nullptr;
        const DropArgs d = make_drop(random && m.p < 1.0f ? m.p : 0.0f, m.seed);
        rm_mark_kernel<<<nblk(N + 1), BS, 0, stream>>>(N, random ? 1 : 0, random && m.p >= 1.0f ? 1 : 0, d, keep);
        GNNMP_LAUNCH_CHECK("rm_mark_kernel");
        if (m.n_remove > 0) {
            rm_list_kernel<<<nblk(m.n_remove), BS, 0, stream>>>(m.remove, m.idx_bytes, m.index_base, m.n_remove, N, keep, meta);
            GNNMP_LAUNCH_CHECK("rm_list_kernel");
        }
    }
    GNNMP_TRY(exclusive_scan_u32(keep, newid, (size_t)N + 1, stream, scan_ws));
    rm_slot_kernel<<<nblk(T + 1), BS, 0, stream>>>(parent->rowptr, parent->col, parent->eid, N, T, E, keep, skeep, ekeep);
    GNNMP_LAUNCH_CHECK("rm_slot_kernel");
    GNNMP_TRY(exclusive_scan_u32(skeep, spos, (size_t)T + 1, stream, scan_ws));
    GNNMP_TRY(exclusive_scan_u32(ekeep, erank, (size_t)E + 1, stream, scan_ws));
    rm_meta_kernel<<<nblk(N), BS, 0, stream>>>(parent->rowptr, N, T, E, keep, newid, spos, erank, meta);
    GNNMP_LAUNCH_CHECK("rm_meta_kernel");
    uint32_t h[META_WORDS] = {};
    GNNMP_HIP(hipMemcpyAsync(h, meta, sizeof(h), hipMemcpyDeviceToHost, stream));
    GNNMP_HIP(hipStreamSynchronize(stream));          // the one synchronisation: the totals size the child
    if (h[META_BAD])
        return fail(GNNMP_EBOUNDS, "%s: a listed node is outside the %lld nodes of the graph", who, (long long)N);
    const int64_t n_keep = h[META_NKEEP], e_keep = h[META_EKEEP], n_slots = h[META_SLOTS];
    if (n_slots != e_keep + (loops ? n_keep : 0))
        return fail(GNNMP_EINVAL, "%s: the parent plan is inconsistent (%lld slots kept for %lld edges and %lld nodes)", who,
                    (long long)n_slots, (long long)e_keep, (long long)n_keep);
    total[0] = n_keep;
    total[1] = e_keep;

    gnnmp_graph_t *c = nullptr;
    GNNMP_TRY(pooled_plan_alloc(&c, n_keep, n_slots, loops, stream));
    RmFill a;
    a.rowptr = parent->rowptr; a.col = parent->col; a.eid = parent->eid;
    a.N = N; a.T = T; a.E = E;
    a.keep = keep; a.newid = newid; a.skeep = skeep; a.spos = spos; a.ekeep = ekeep; a.erank = erank;
    a.n_keep = (uint32_t)n_keep; a.e_keep = (uint32_t)e_keep; a.n_slots = (uint32_t)n_slots;
    a.rowptr_out = c->rowptr; a.col_out = c->col; a.eid_out = c->eid;
    a.node_map = node_map_out; a.node_new = node_new_out; a.edge_map = edge_map_out;
    a.row_blocks = nblk(N + 1);
    a.slot_blocks = T > 0 ? nblk(T) : 0u;
    const unsigned edge_blocks = edge_map_out && E > 0 ? nblk(E) : 0u;
    hipError_t e = hipMemsetAsync(c->status, 0, 4 * sizeof(int32_t), stream);
    if (e == hipSuccess) {
        rm_fill_kernel<<<a.row_blocks + a.slot_blocks + edge_blocks, BS, 0, stream>>>(a);
        e = hipGetLastError();
    }
    int rc = e == hipSuccess ? GNNMP_OK : hip_fail(e, "rm_fill_kernel");
    c->max_degree = (int64_t)h[META_MAXDEG];
    // (hub rows that stay long: the chunk tables, with a synchronisation, as every plan build makes them)
    if (rc == GNNMP_OK && c->max_degree > c->long_thresh) rc = plan_build_long_rows(c, stream);
    if (rc != GNNMP_OK) {
        plan_dispose(c, stream, true);
        return rc;
    }
    *out = c;
    return GNNMP_OK;
}

}  // namespace
}  // namespace gnnmp

using namespace gnnmp;

extern "C" {

int gnnmp_plan_remove_nodes(gnnmp_graph_t **out, const gnnmp_graph_t *parent, const void *remove, int idx_bytes, int index_base,
                            int64_t n_remove, float p, uint64_t seed, int32_t *node_map_out, int32_t *node_new_out,
                            uint32_t *edge_map_out, int64_t *total, gnnmp_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    GNNMP_TRY(check_common("plan_remove_nodes", out, parent, idx_bytes, index_base));
    if (!total) return fail(GNNMP_EINVAL, "plan_remove_nodes: total is NULL");
    total[0] = total[1] = 0;
    if (n_remove < 0) return fail(GNNMP_EINVAL, "plan_remove_nodes: negative n_remove");
    if (!(p >= 0.0f && p <= 1.0f)) return fail(GNNMP_EINVAL, "plan_remove_nodes: probability %g outside [0, 1]", (double)p);
    if (remove && p != 0.0f) return fail(GNNMP_EINVAL, "plan_remove_nodes: a remove list and a probability (p must be 0 in list mode)");
    if (!remove && n_remove != 0) return fail(GNNMP_EINVAL, "plan_remove_nodes: n_remove = %lld without a remove list", (long long)n_remove);
    RmMark m;
    m.remove = remove; m.idx_bytes = idx_bytes; m.index_base = index_base; m.n_remove = n_remove; m.p = p; m.seed = seed;
    return rm_derive("plan_remove_nodes", out, parent, m, node_map_out, node_new_out, edge_map_out, total, stream);
}

int gnnmp_plan_keep_nodes(gnnmp_graph_t **out, const gnnmp_graph_t *parent, const uint32_t *keep, int32_t *node_map_out,
                          int32_t *node_new_out, uint32_t *edge_map_out, int64_t *total, gnnmp_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    GNNMP_TRY(check_common("plan_keep_nodes", out, parent, 8, 0));
    if (!total) return fail(GNNMP_EINVAL, "plan_keep_nodes: total is NULL");
    total[0] = total[1] = 0;
    if (!keep && parent->n_dst > 0) return fail(GNNMP_EINVAL, "plan_keep_nodes: keep is NULL");
    RmMark m;
    m.by_mask = true;
    m.mask = keep;      // (NULL only with N = 0: never read)
    return rm_derive("plan_keep_nodes", out, parent, m, node_map_out, node_new_out, edge_map_out, total, stream);
}

int gnnmp_plan_add_edges(gnnmp_graph_t **out, const gnnmp_graph_t *parent, const void *s_new, const void *t_new, int idx_bytes,
                         int index_base, int64_t m, int64_t n_nodes, uint64_t seed, void *s_new_out, void *t_new_out,
                         gnnmp_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    GNNMP_TRY(check_common("plan_add_edges", out, parent, idx_bytes, index_base));
    const int64_t N = parent->n_dst, T = parent->n_total, E = parent->n_edges;
    const int loops = parent->self_loops;
    if (m < 0) return fail(GNNMP_EINVAL, "plan_add_edges: negative m");
    if (n_nodes < N) return fail(GNNMP_EINVAL, "plan_add_edges: n_nodes = %lld below the parent's %lld nodes", (long long)n_nodes, (long long)N);
    if ((s_new == nullptr) != (t_new == nullptr)) return fail(GNNMP_EINVAL, "plan_add_edges: s_new and t_new go together");
    const bool random = s_new == nullptr;
    if (random && m > 0) {
        if (!s_new_out || !t_new_out) return fail(GNNMP_EINVAL, "plan_add_edges: random mode needs s_new_out and t_new_out");
        if (N < 2) return fail(GNNMP_EINVAL, "plan_add_edges: Graph must contain at least 2 nodes to add edges (it has %lld)", (long long)N);
    }
    const int64_t n_slots = T + m + (loops ? n_nodes - N : 0);
    if (m >= (int64_t)GNNMP_MAX_SLOTS || n_slots >= (int64_t)GNNMP_MAX_SLOTS || n_nodes >= (int64_t)INT32_MAX)
        return fail(GNNMP_EUNSUPPORTED, "plan_add_edges: E' = %lld (limit 2^32 - 65536) / N = %lld (limit 2^31 - 2) exceed the plan format",
                    (long long)n_slots, (long long)n_nodes);

    // scratch: keys_in | keys_out | vals_in | vals_out | snew [m], newptr [n_nodes + 1], the bad-index word
    const size_t nM = up64((size_t)std::max<int64_t>(m, 1)), nP = up64((size_t)n_nodes + 1);
    PoolScratch sc(stream);
    const size_t words = 5 * nM + nP + 64;
    if (!sc.take(sizeof(uint32_t) * words)) return fail(GNNMP_EALLOC, "plan_add_edges: hipMalloc of %zu bytes failed", 4 * words);
    uint32_t *const keys_in = static_cast<uint32_t *>(sc.p), *const keys_out = keys_in + nM, *const vals_in = keys_out + nM,
                   *const vals_out = vals_in + nM, *const newptr = vals_out + 2 * nM, *const bad = newptr + nP;
    int32_t *const snew = reinterpret_cast<int32_t *>(vals_out + nM);
    if (m > 0) {
        GNNMP_HIP(hipMemsetAsync(bad, 0, sizeof(uint32_t), stream));
        ae_keys_kernel<<<nblk(m), BS, 0, stream>>>(s_new, t_new, idx_bytes, index_base, m, N, n_nodes, (uint32_t)seed,
                                                   (uint32_t)(seed >> 32), s_new_out, t_new_out, keys_in, vals_in, snew, bad);
        GNNMP_LAUNCH_CHECK("ae_keys_kernel");
        // stable LSD radix sort of (destination, position) of the NEW edges, on the bits that can be set (synchronises the stream)
        unsigned bits = 1;
        while (bits < 32 && ((int64_t)1 << bits) < n_nodes) ++bits;
        GNNMP_TRY(radix_sort_pairs_u32(keys_in, keys_out, vals_in, vals_out, (size_t)m, 0, (int)bits, stream));
        if (!random) {
            uint32_t hbad = 0;
            GNNMP_HIP(hipMemcpyAsync(&hbad, bad, sizeof(hbad), hipMemcpyDeviceToHost, stream));
            GNNMP_HIP(hipStreamSynchronize(stream));
            if (hbad)
                return fail(GNNMP_EBOUNDS, "plan_add_edges: a new edge's index is outside the %lld nodes of the child", (long long)n_nodes);
        }
    }
    ae_newptr_kernel<<<nblk(n_nodes + 1), BS, 0, stream>>>(keys_out, m, n_nodes, newptr);
    GNNMP_LAUNCH_CHECK("ae_newptr_kernel");

    gnnmp_graph_t *c = nullptr;
    GNNMP_TRY(pooled_plan_alloc(&c, n_nodes, n_slots, loops, stream));
    AeFill a;
    a.rowptr = parent->rowptr; a.col = parent->col; a.eid = parent->eid;
    a.N = N; a.T = T; a.E = E; a.m = m; a.n_nodes = n_nodes;
    a.loops = loops;
    a.keys = keys_out; a.vals = vals_out; a.newptr = newptr; a.snew = snew;
    a.rowptr_out = c->rowptr; a.col_out = c->col; a.eid_out = c->eid;
    a.row_blocks = nblk(n_nodes + 1);
    a.slot_blocks = T > 0 ? nblk(T) : 0u;
    const unsigned new_blocks = m > 0 ? nblk(m) : 0u;
    hipError_t e = hipMemsetAsync(c->status, 0, 4 * sizeof(int32_t), stream);
    if (e == hipSuccess) {
        ae_fill_kernel<<<a.row_blocks + a.slot_blocks + new_blocks, BS, 0, stream>>>(a);
        e = hipGetLastError();
    }
    int rc = e == hipSuccess ? GNNMP_OK : hip_fail(e, "ae_fill_kernel");
    // the child's longest row and, above its threshold, the chunk tables (synchronises the stream, as gnnmp_plan_create does)
    if (rc == GNNMP_OK) rc = plan_build_long_rows(c, stream);
    if (rc != GNNMP_OK) {
        plan_dispose(c, stream, true);
        return rc;
    }
    *out = c;
    return GNNMP_OK;
}

}  // extern "C"
