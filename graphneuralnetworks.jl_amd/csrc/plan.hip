// plan.hip — graph-side prep: dst-sorted CSR plan of a COO edge index, plus the bit-exact index ops
// (add_self_loops, batch).  Reference: GNNGraphs/src/gnngraph.jl:108-117 (COO container),
// GNNGraphs/src/convert.jl:221-237 (to_sparse, rebuilt per call by the reference fast path),
// GNNGraphs/src/transform.jl:12-28 (add_self_loops), :682-709 (batch).
#include <cstring>
#include <algorithm>
#include <vector>

#include "common.h"
#include "launch.h"
#include "pool.h"
#include "scratch.h"
#include "sort_scan.h"

namespace gnnmp {

int ensure_workspace(gnnmp_graph *p, size_t floats) { return grow(p->ws, p->ws_floats, floats, "hipMalloc(plan workspace)"); }

int ensure_arrive(gnnmp_graph *p, size_t n, size_t floats, hipStream_t stream) {
    GNNMP_TRY(grow(p->spart, p->spart_floats, floats, "hipMalloc(plan slice partials)"));
    if (n <= p->arrive_n) return GNNMP_OK;
    // (counters are zero between launches, nothing to carry over)
    GNNMP_TRY(grow(p->arrive, p->arrive_n, n, "hipMalloc(plan arrival counters)"));
    const hipError_t e = hipMemsetAsync(p->arrive, 0, sizeof(uint32_t) * n, stream);
    if (e != hipSuccess) {
        p->arrive_n = 0;   // not zeroed: the next call starts over
        return hip_fail(e, "hipMemsetAsync(plan arrival counters)");
    }
    return GNNMP_OK;
}

int ensure_ticket(gnnmp_graph *p, hipStream_t stream) {
    if (p->ticket) return GNNMP_OK;
    size_t cap = 0;
    GNNMP_TRY(grow(p->ticket, cap, 2, "hipMalloc(plan ticket)"));
    const hipError_t e = hipMemsetAsync(p->ticket, 0, 2 * sizeof(uint32_t), stream);
    if (e != hipSuccess) return hip_fail(e, "hipMemsetAsync(plan ticket)");
    return GNNMP_OK;
}

__global__ void plan_degree_keys(const uint32_t *rowptr, int64_t n, uint32_t maxdeg, uint32_t *keys, uint32_t *vals) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    keys[i] = maxdeg - (rowptr[i + 1] - rowptr[i]);   // ascending key = descending length
    vals[i] = (uint32_t)i;
}

int ensure_row_order(gnnmp_graph *p, hipStream_t stream) {
    if (p->row_order || p->n_dst == 0) return GNNMP_OK;
    const size_t n = (size_t)p->n_dst;
    unsigned bits = 1;
    while (bits < 32 && ((int64_t)1 << bits) <= p->max_degree) ++bits;   // max_degree <= E' < 2^32
    DevBuf<int32_t> order;
    DevBuf<uint32_t> vin, kout, kin;
    hipError_t e = hipSuccess;
    if ((e = kin.alloc(n)) != hipSuccess || (e = kout.alloc(n)) != hipSuccess || (e = vin.alloc(n)) != hipSuccess ||
        (e = order.alloc(n)) != hipSuccess)
        return hip_fail(e, "hipMalloc(row order)");
    plan_degree_keys<<<(unsigned)((n + 255) / 256), 256, 0, stream>>>(p->rowptr, p->n_dst, (uint32_t)p->max_degree, kin.get(), vin.get());
    GNNMP_TRY(radix_sort_pairs_u32(kin.get(), kout.get(), vin.get(), reinterpret_cast<uint32_t *>(order.get()), n, 0, (int)bits,
                                   stream));   // syncs the stream
    p->row_order = order.release();
    p->bytes += (int64_t)(4 * n);
    return GNNMP_OK;
}

// ---- kernels -----------------------------------------------------------------------------------

// keys[k] = 0-based destination of edge k (self loops k >= E: k - E); vals[k] = k.
// bad[0] is set if any index is outside its range.
__global__ void plan_fill_keys(const void *src, const void *dst, int idx_bytes, int base, int64_t E,
                               int64_t Etot, int64_t n_src, int64_t n_dst, uint32_t *keys,
                               uint32_t *vals, int *bad) {
    int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= Etot) return;
    int64_t d;
    if (k < E) {
        d = load_index(dst, k, idx_bytes, base);
        int64_t s = load_index(src, k, idx_bytes, base);
        if (d < 0 || d >= n_dst || s < 0 || s >= n_src) {
            *bad = 1;
            d = 0;
        }
    } else {
        d = k - E;
    }
    keys[k] = (uint32_t)d;
    vals[k] = (uint32_t)k;
}

// rowptr[i] = first slot whose key >= i  (binary search in the sorted keys); rowptr[n_dst] = Etot
__global__ void plan_rowptr(const uint32_t *keys, int64_t Etot, int64_t n_dst, uint32_t *rowptr) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n_dst) return;
    int64_t lo = 0, hi = Etot;
    while (lo < hi) {
        int64_t mid = (lo + hi) >> 1;
        if ((int64_t)keys[mid] < i)
            lo = mid + 1;
        else
            hi = mid;
    }
    rowptr[i] = (uint32_t)lo;
}

// col[p] = 0-based source of the edge in slot p
__global__ void plan_col(const void *src, int idx_bytes, int base, int64_t E, int64_t Etot,
                         const uint32_t *eid, int32_t *col) {
    int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= Etot) return;
    int64_t e = eid[p];
    int64_t s = e < E ? load_index(src, e, idx_bytes, base) : e - E;
    col[p] = (int32_t)s;
}

// ---- a plan straight from a compressed-sparse-column adjacency (gnnmp_plan_from_csc): no sort ---------------------------------------
// rowptr[i] = colptr[i] - base; flags[0] |= 1 if the column pointers do not start at `base`, end at E + base or decrease
__global__ void csc_rowptr_kernel(const void *colptr, int idx_bytes, int base, int64_t n_dst, int64_t E, uint32_t *rowptr, int *bad) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n_dst) return;
    const int64_t v = load_index(colptr, i, idx_bytes, base);
    bool ok = v >= 0 && v <= E;
    if (i == 0) ok = ok && v == 0;
    if (i == n_dst) ok = ok && v == E;
    if (i < n_dst) ok = ok && load_index(colptr, i + 1, idx_bytes, base) >= v;
    if (!ok) *bad = 1;
    rowptr[i] = (uint32_t)(ok ? v : (i == n_dst ? E : 0));
}
// col[p] = rowval[p] - base, eid[p] = p (findnz order IS the slot order); flags[0] |= 1 for a source outside the graph
__global__ void csc_col_kernel(const void *rowval, int idx_bytes, int base, int64_t E, int64_t n_src, int32_t *col, int32_t *eid, int *bad) {
    int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= E) return;
    int64_t s = load_index(rowval, p, idx_bytes, base);
    if (s < 0 || s >= n_src) {
        *bad = 1;
        s = 0;
    }
    col[p] = (int32_t)s;
    eid[p] = (int32_t)(uint32_t)p;
}

// collect rows longer than `thresh` as (row, beg, end) triples; *count = how many (atomic), *maxdeg = max degree
__global__ void plan_long_rows(const uint32_t *rowptr, int64_t n_dst, int thresh, int64_t *list,
                               int cap, int *count, unsigned long long *maxdeg) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_dst) return;
    const int64_t beg = rowptr[i], end = rowptr[i + 1];
    const int64_t len = end - beg;
    if (len > 0) atomicMax(maxdeg, (unsigned long long)len);
    if (len > thresh) {
        int pos = atomicAdd(count, 1);
        if (pos < cap) {
            list[3 * pos] = i;
            list[3 * pos + 1] = beg;
            list[3 * pos + 2] = end;
        }
    }
}
__global__ void widen_u32_kernel(const uint32_t *in, int64_t n, int64_t *out) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = (int64_t)in[i];
}

// out[p] = v[col[p]] (by == 0, node vector) or v[eid[p]] with 1.0 for plan-added self loops (by == 1, edge vector)
__global__ void slot_gather_kernel(const int32_t *idx, const float *v, int64_t Etot, int64_t n_valid,
                                   float *out) {
    int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= Etot) return;
    const int64_t k = (uint32_t)idx[p];   // source ids (< 2^31) or edge positions (< 2^32): unsigned either way
    out[p] = k < n_valid ? v[k] : 1.0f;
}

__global__ void self_loops_kernel(const void *src, const void *dst, int idx_bytes, int base,
                                  int64_t E, int64_t n, void *out_src, void *out_dst,
                                  const float *w, float *out_w) {
    int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= E + n) return;
    if (k < E) {
        store_index(out_src, k, idx_bytes, load_index(src, k, idx_bytes, 0));
        store_index(out_dst, k, idx_bytes, load_index(dst, k, idx_bytes, 0));
        if (out_w) out_w[k] = w[k];
    } else {
        int64_t v = (k - E) + base;
        store_index(out_src, k, idx_bytes, v);
        store_index(out_dst, k, idx_bytes, v);
        if (out_w) out_w[k] = 1.0f;
    }
}

// one thread per edge: find its graph by binary search in edge_ptr, add the node offset.
__global__ void batch_edges_kernel(const void *src, const void *dst, int idx_bytes,
                                   const int64_t *edge_ptr, const int64_t *node_ptr, int64_t G,
                                   int64_t Etot, void *out_src, void *out_dst) {
    int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= Etot) return;
    int64_t lo = 0, hi = G;  // largest g with edge_ptr[g] <= k
    while (hi - lo > 1) {
        int64_t mid = (lo + hi) >> 1;
        if (edge_ptr[mid] <= k)
            lo = mid;
        else
            hi = mid;
    }
    int64_t off = node_ptr[lo];
    store_index(out_src, k, idx_bytes, load_index(src, k, idx_bytes, 0) + off);
    store_index(out_dst, k, idx_bytes, load_index(dst, k, idx_bytes, 0) + off);
}
__global__ void batch_indicator_kernel(const int64_t *node_ptr, int64_t G, int64_t Ntot,
                                       int idx_bytes, int base, void *gi) {
    int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= Ntot) return;
    int64_t lo = 0, hi = G;
    while (hi - lo > 1) {
        int64_t mid = (lo + hi) >> 1;
        if (node_ptr[mid] <= v)
            lo = mid;
        else
            hi = mid;
    }
    store_index(gi, v, idx_bytes, lo + base);
}

static inline unsigned nblocks(int64_t n, int bs) { return (unsigned)((n + bs - 1) / bs); }

// Long-row threshold: a row is reduced sequentially by one lane group, ~0.25 us per edge once HBM latency is the
// limit, while the whole kernel moves an edge every ~0.1 ns; rows above ~4e-5 * E' edges would become the tail.
// Clamped to [GNNMP_MIN_LONG_ROW, GNNMP_LONG_ROW]; rows up to this length keep the exact reference edge order.
int plan_long_thresh(int64_t Etot) {
    if (knob(KNOB_LONG_ROW) > 0) return knob(KNOB_LONG_ROW);
    int th = GNNMP_MIN_LONG_ROW;
    while (th < GNNMP_LONG_ROW && (double)th < 4e-5 * (double)Etot) th <<= 1;
    return th;
}

// slots per chunk of a split row (<= the plan's long_thresh): 128, or KNOB_CHUNK_SLOTS from 16 up (A/B runs)
static int plan_chunk_slots() {
    const int v = knob(KNOB_CHUNK_SLOTS);
    return v >= 16 ? v : 128;
}

int plan_build_long_rows(gnnmp_graph *p, hipStream_t stream) {
    const int64_t n_dst = p->n_dst, Etot = p->n_total;
    const int BS = 256;
    // long rows: at most Etot / thresh of them
    const int cap = (int)std::min<int64_t>(Etot / std::max(1, p->long_thresh) + 1, n_dst + 1);
    DevBuf<int64_t> long_tmp;
    DevBuf<int> flags;       // [0] long count; [2..3] = one unsigned long long: max degree
    GNNMP_HIP(flags.alloc(4));
    GNNMP_HIP(hipMemsetAsync(flags.get(), 0, sizeof(int) * 4, stream));
    GNNMP_HIP(long_tmp.alloc(3 * (size_t)std::max(cap, 1)));
    if (n_dst > 0) {
        plan_long_rows<<<nblocks(n_dst, BS), BS, 0, stream>>>(p->rowptr, n_dst, p->long_thresh, long_tmp.get(), cap, flags.get(),
                                                              reinterpret_cast<unsigned long long *>(flags.get() + 2));
        GNNMP_HIP(hipGetLastError());
    }
    int meta[4] = {0, 0, 0, 0};
    GNNMP_HIP(hipMemcpyAsync(meta, flags.get(), sizeof(int) * 4, hipMemcpyDeviceToHost, stream));
    GNNMP_HIP(hipStreamSynchronize(stream));
    unsigned long long md;
    memcpy(&md, meta + 2, sizeof(md));
    p->max_degree = (int64_t)md;
    p->n_long = std::min(meta[0], cap);
    if (p->n_long == 0) return GNNMP_OK;
    struct Tri { int64_t row, beg, end; };
    std::vector<Tri> h((size_t)p->n_long);
    GNNMP_HIP(hipMemcpy(h.data(), long_tmp.get(), sizeof(Tri) * h.size(), hipMemcpyDeviceToHost));
    // atomics filled the list in arbitrary order: make it canonical (ascending row)
    std::sort(h.begin(), h.end(), [](const Tri &a, const Tri &b) { return a.row < b.row; });
    std::vector<int32_t> rows, cptr, crow, clrow;
    std::vector<uint32_t> cbeg, cend;
    cptr.push_back(0);
    // Chunk length (round 6): rows are split ABOVE long_thresh (that is what bounds bit-exactness and keeps a sequential row from
    // being the kernel's tail), but the chunks of a row that is split anyway are at most plan_chunk_slots() = 128 slots long: a chunk
    // is a latency-bound chain of len / 8 row-load batches, and the fused layer kernel's pre-pass over the split rows — nothing
    // else runs beside it — took 110 us of a 4.8 ms GCN layer with 512-slot chunks on the products shape.
    const int64_t clen = std::min<int64_t>(p->long_thresh, plan_chunk_slots());
    for (const Tri &t : h) {
        const int64_t len = t.end - t.beg;
        const int64_t nch = (len + clen - 1) / clen;
        const int64_t csz = (len + nch - 1) / nch;  // balanced chunks, each <= clen <= long_thresh slots
        for (int64_t c = 0; c < nch; ++c) {
            crow.push_back((int32_t)t.row);
            clrow.push_back((int32_t)rows.size());
            cbeg.push_back((uint32_t)(t.beg + c * csz));
            cend.push_back((uint32_t)std::min(t.beg + (c + 1) * csz, t.end));
        }
        rows.push_back((int32_t)t.row);
        cptr.push_back((int32_t)crow.size());
    }
    if (crow.size() >= (size_t)INT32_MAX)
        return fail(GNNMP_EUNSUPPORTED, "plan_create: %zu chunks of split rows exceed the int32 chunk index", crow.size());
    p->n_chunks = (int)crow.size();
    auto upload = [&](auto *&dst, const auto &v) -> hipError_t {
        const size_t bytes = sizeof(v[0]) * v.size();
        const hipError_t e = alloc_into(dst, v.size());
        if (e != hipSuccess) return e;
        p->bytes += (int64_t)bytes;
        return hipMemcpy(dst, v.data(), bytes, hipMemcpyHostToDevice);
    };
    GNNMP_HIP(upload(p->long_rows, rows));
    GNNMP_HIP(upload(p->long_cptr, cptr));
    // (16 bytes of p->bytes per chunk, the four arrays below: tests/test_chunk_slots.py reads the chunk count of a plan off gnnmp_plan_info's bytes)
    GNNMP_HIP(upload(p->chunk_row, crow));
    GNNMP_HIP(upload(p->chunk_lrow, clrow));
    GNNMP_HIP(upload(p->chunk_beg, cbeg));
    GNNMP_HIP(upload(p->chunk_end, cend));
    return GNNMP_OK;
}

}  // namespace gnnmp

using namespace gnnmp;

extern "C" {

int gnnmp_plan_destroy(gnnmp_graph_t *p) { return plan_dispose(p, nullptr, false); }

/* the arrival counters of the in-kernel fold and the fused layer kernel's ticket back to zero, stream-ordered (gnnmp.h: repair hook) */
int gnnmp_plan_reset_counters(gnnmp_graph_t *p, gnnmp_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!p) return fail(GNNMP_EINVAL, "plan_reset_counters: null plan");
    if (p->arrive && p->arrive_n) GNNMP_HIP(hipMemsetAsync(p->arrive, 0, sizeof(uint32_t) * p->arrive_n, stream));
    if (p->ticket) GNNMP_HIP(hipMemsetAsync(p->ticket, 0, 2 * sizeof(uint32_t), stream));
    return GNNMP_OK;
}

/* stream-ordered destroy of a pooled plan (gnnmp_plan_concat / gnnmp_plan_select): see gnnmp.h */
int gnnmp_plan_release(gnnmp_graph_t *p, gnnmp_stream_t stream) { return plan_dispose(p, (hipStream_t)stream, true); }

}  // extern "C"

namespace gnnmp {
int plan_dispose(gnnmp_graph_t *p, hipStream_t stream, bool stream_known) {
    if (!p) return GNNMP_OK;
    if (p->block) {
        // rowptr / col / eid are pieces of the pooled block: back to the pool (with an event on `stream` when the caller names it)
        pool_park(p->block, p->block_bytes, stream, stream_known);
        p->rowptr = nullptr;
        p->col = nullptr;
        p->eid = nullptr;
    }
    void *const owned[] = {p->rowptr, p->col, p->eid, p->long_rows, p->long_cptr, p->chunk_row, p->chunk_lrow, p->arrive, p->spart,
                           p->chunk_beg, p->chunk_end, p->ws, p->ticket, p->row_order};
    for (void *q : owned)
        if (q) (void)dev_free(q);
    delete p;
    return GNNMP_OK;
}
int check_transposed(const char *who, const gnnmp_graph_t *plan, const gnnmp_graph_t *plan_t) {
    if (plan_t->n_dst != plan->n_src || plan_t->n_src != plan->n_dst || plan_t->n_total != plan->n_total)
        return fail(GNNMP_EINVAL, "%s: plan_t is not the transpose of plan (%lld x %lld, %lld edges vs %lld x %lld, %lld)", who,
                    (long long)plan_t->n_dst, (long long)plan_t->n_src, (long long)plan_t->n_total,
                    (long long)plan->n_dst, (long long)plan->n_src, (long long)plan->n_total);
    return GNNMP_OK;
}
int check_edge_plan(const char *who, const gnnmp_graph_t *plan, const gnnmp_graph_t *plan_t, bool need_square, const char *no_row) {
    if (need_square && plan->n_src != plan->n_dst)
        return fail(GNNMP_EINVAL, "%s: the plan is not square (%lld sources, %lld destinations)", who, (long long)plan->n_src,
                    (long long)plan->n_dst);
    if (plan_t) {
        if (plan_t->n_dst != plan->n_dst || plan_t->n_src != plan->n_src)
            return fail(GNNMP_EINVAL, "%s: the transposed plan has %lld rows, the plan %lld", who, (long long)plan_t->n_dst,
                        (long long)plan->n_dst);
        if (plan_t->n_edges != plan->n_edges || plan_t->n_total != plan->n_total)
            return fail(GNNMP_EINVAL, "%s: the transposed plan has %lld edges, the plan %lld", who, (long long)plan_t->n_total,
                        (long long)plan->n_total);
    }
    if (no_row && plan->n_total != plan->n_edges)
        return fail(GNNMP_EINVAL, "%s: the plan was built with self loops (%lld slots, %lld edges): %s", who, (long long)plan->n_total,
                    (long long)plan->n_edges, no_row);
    return GNNMP_OK;
}
}  // namespace gnnmp

extern "C" {

int gnnmp_plan_create(gnnmp_graph_t **out, const void *src, const void *dst, int idx_bytes,
                      int index_base, int64_t n_src, int64_t n_dst, int64_t n_edges,
                      int add_self_loops, int validate, gnnmp_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!out) return fail(GNNMP_EINVAL, "plan_create: out is NULL");
    *out = nullptr;
    if (idx_bytes != 4 && idx_bytes != 8)
        return fail(GNNMP_EINVAL, "plan_create: idx_bytes must be 4 or 8 (got %d)", idx_bytes);
    if (index_base != 0 && index_base != 1)
        return fail(GNNMP_EINVAL, "plan_create: index_base must be 0 or 1 (got %d)", index_base);
    if (n_src < 0 || n_dst < 0 || n_edges < 0)
        return fail(GNNMP_EINVAL, "plan_create: negative size");
    if (n_edges > 0 && (!src || !dst)) return fail(GNNMP_EINVAL, "plan_create: null edge index");
    if (add_self_loops && n_src != n_dst)
        return fail(GNNMP_EINVAL, "plan_create: add_self_loops needs n_src == n_dst (%lld vs %lld)",
                    (long long)n_src, (long long)n_dst);
    const int64_t Etot = n_edges + (add_self_loops ? n_dst : 0);
    // slots and edge positions are UNSIGNED 32-bit, node ids signed 32-bit; 65 536 slots of headroom so that no slot counter of
    // a kernel (base += G, p0 += 4, off += cap ...) can wrap
    if (Etot >= (int64_t)GNNMP_MAX_SLOTS || n_src >= (int64_t)INT32_MAX || n_dst >= (int64_t)INT32_MAX)
        return fail(GNNMP_EUNSUPPORTED, "plan_create: E' = %lld (limit 2^32 - 65536) / N = %lld (limit 2^31 - 2) exceed the plan format",
                    (long long)Etot, (long long)std::max(n_src, n_dst));

    PlanPtr p(new gnnmp_graph_t());
    p->n_src = n_src;
    p->n_dst = n_dst;
    p->n_edges = n_edges;
    p->n_total = Etot;
    p->self_loops = add_self_loops ? 1 : 0;
    p->long_thresh = plan_long_thresh(Etot);

    const int BS = 256;
    const size_t epad = (size_t)std::max<int64_t>(Etot, 1);
    DevBuf<int> flags;                  // [0] bad index
    DevBuf<unsigned char> sort_keys;    // keys_in | keys_out | vals_in: one allocation for the three key / value arrays of the sort
    uint32_t *keys_out = nullptr;
    GNNMP_HIP(alloc_into(p->rowptr, (size_t)(n_dst + 1)));
    GNNMP_HIP(alloc_into(p->col, epad));
    GNNMP_HIP(alloc_into(p->eid, epad));
    GNNMP_HIP(flags.alloc(4));
    GNNMP_HIP(hipMemsetAsync(flags.get(), 0, sizeof(int) * 4, stream));
    p->bytes = (int64_t)(sizeof(int32_t) * ((size_t)(n_dst + 1) + 2 * epad));

    if (Etot > 0) {
        const size_t piece = (sizeof(uint32_t) * epad + 255) & ~(size_t)255;
        GNNMP_HIP(sort_keys.alloc(3 * piece));
        uint32_t *keys_in = reinterpret_cast<uint32_t *>(sort_keys.get());
        keys_out = reinterpret_cast<uint32_t *>(sort_keys.get() + piece);
        uint32_t *vals_in = reinterpret_cast<uint32_t *>(sort_keys.get() + 2 * piece);
        plan_fill_keys<<<nblocks(Etot, BS), BS, 0, stream>>>(src, dst, idx_bytes, index_base,
                                                             n_edges, Etot, n_src, n_dst, keys_in,
                                                             vals_in, flags.get());
        GNNMP_HIP(hipGetLastError());
        if (validate) {
            int bad = 0;
            GNNMP_HIP(hipMemcpyAsync(&bad, flags.get(), sizeof(int), hipMemcpyDeviceToHost, stream));
            GNNMP_HIP(hipStreamSynchronize(stream));
            if (bad)
                return fail(GNNMP_EBOUNDS, "plan_create: edge index outside 1..N (n_src=%lld n_dst=%lld)",
                            (long long)n_src, (long long)n_dst);
        }
        // stable LSD radix sort of (dst, edge position) on the bits that can be set
        unsigned bits = 1;
        while (bits < 32 && ((int64_t)1 << bits) < n_dst) ++bits;
        GNNMP_TRY(radix_sort_pairs_u32(keys_in, keys_out, vals_in, reinterpret_cast<uint32_t *>(p->eid), (size_t)Etot, 0, (int)bits,
                                       stream));
        plan_col<<<nblocks(Etot, BS), BS, 0, stream>>>(src, idx_bytes, index_base, n_edges, Etot,
                                                       reinterpret_cast<uint32_t *>(p->eid), p->col);
        GNNMP_HIP(hipGetLastError());
    }
    plan_rowptr<<<nblocks(n_dst + 1, BS), BS, 0, stream>>>(keys_out, Etot, n_dst, p->rowptr);
    GNNMP_HIP(hipGetLastError());

    GNNMP_TRY(plan_build_long_rows(p.get(), stream));
    *out = p.release();
    return GNNMP_OK;
}

int gnnmp_plan_from_csc(gnnmp_graph_t **out, const void *colptr, const void *rowval, int idx_bytes, int index_base, int64_t n_src,
                        int64_t n_dst, int64_t n_edges, int validate, gnnmp_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!out) return fail(GNNMP_EINVAL, "plan_from_csc: out is NULL");
    *out = nullptr;
    if (idx_bytes != 4 && idx_bytes != 8) return fail(GNNMP_EINVAL, "plan_from_csc: idx_bytes must be 4 or 8 (got %d)", idx_bytes);
    if (index_base != 0 && index_base != 1) return fail(GNNMP_EINVAL, "plan_from_csc: index_base must be 0 or 1 (got %d)", index_base);
    if (n_src < 0 || n_dst < 0 || n_edges < 0) return fail(GNNMP_EINVAL, "plan_from_csc: negative size");
    if (!colptr || (n_edges > 0 && !rowval)) return fail(GNNMP_EINVAL, "plan_from_csc: null colptr / rowval");
    if (n_edges >= (int64_t)GNNMP_MAX_SLOTS || n_src >= (int64_t)INT32_MAX || n_dst >= (int64_t)INT32_MAX)
        return fail(GNNMP_EUNSUPPORTED, "plan_from_csc: E = %lld (limit 2^32 - 65536) / N = %lld (limit 2^31 - 2) exceed the plan format",
                    (long long)n_edges, (long long)std::max(n_src, n_dst));
    PlanPtr p(new gnnmp_graph_t());
    p->n_src = n_src;
    p->n_dst = n_dst;
    p->n_edges = n_edges;
    p->n_total = n_edges;
    p->long_thresh = plan_long_thresh(n_edges);
    const int BS = 256;
    const size_t epad = (size_t)std::max<int64_t>(n_edges, 1);
    DevBuf<int> flags;
    GNNMP_HIP(alloc_into(p->rowptr, (size_t)(n_dst + 1)));
    GNNMP_HIP(alloc_into(p->col, epad));
    GNNMP_HIP(alloc_into(p->eid, epad));
    GNNMP_HIP(flags.alloc(4));
    GNNMP_HIP(hipMemsetAsync(flags.get(), 0, sizeof(int) * 4, stream));
    p->bytes = (int64_t)(sizeof(int32_t) * ((size_t)(n_dst + 1) + 2 * epad));
    csc_rowptr_kernel<<<nblocks(n_dst + 1, BS), BS, 0, stream>>>(colptr, idx_bytes, index_base, n_dst, n_edges, p->rowptr, flags.get());
    GNNMP_HIP(hipGetLastError());
    if (n_edges > 0) {
        csc_col_kernel<<<nblocks(n_edges, BS), BS, 0, stream>>>(rowval, idx_bytes, index_base, n_edges, n_src, p->col, p->eid, flags.get());
        GNNMP_HIP(hipGetLastError());
    }
    (void)validate;
    // ALWAYS checked: the build synchronises below anyway (plan_build_long_rows), so skipping the read-back would save nothing, and a
    // column pointer sanitised entry by entry can leave a row with beg > end that no kernel would ever write
    int bad = 0;
    GNNMP_HIP(hipMemcpyAsync(&bad, flags.get(), sizeof(int), hipMemcpyDeviceToHost, stream));
    GNNMP_HIP(hipStreamSynchronize(stream));
    if (bad)
        return fail(GNNMP_EBOUNDS, "plan_from_csc: colptr is not a monotone 0..E column pointer, or a row index lies outside 1..n_src "
                    "(n_src=%lld n_dst=%lld E=%lld)", (long long)n_src, (long long)n_dst, (long long)n_edges);
    GNNMP_TRY(plan_build_long_rows(p.get(), stream));
    *out = p.release();
    return GNNMP_OK;
}

int gnnmp_plan_slot_gather_f32(gnnmp_graph_t *p, int by, const float *v, float *out_slot,
                               gnnmp_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!p) return fail(GNNMP_EINVAL, "plan_slot_gather: null plan");
    if (by != 0 && by != 1) return fail(GNNMP_EINVAL, "plan_slot_gather: `by` must be 0 (node) or 1 (edge)");
    if (p->n_total == 0) return GNNMP_OK;
    if (!v || !out_slot) return fail(GNNMP_EINVAL, "plan_slot_gather: null pointer");
    if (by == 0)
        slot_gather_kernel<<<nblocks(p->n_total, 256), 256, 0, stream>>>(p->col, v, p->n_total, p->n_src, out_slot);
    else
        slot_gather_kernel<<<nblocks(p->n_total, 256), 256, 0, stream>>>(p->eid, v, p->n_total, p->n_edges, out_slot);
    GNNMP_LAUNCH_CHECK("slot_gather_kernel");
    return GNNMP_OK;
}

int gnnmp_plan_info(const gnnmp_graph_t *p, int64_t info[8]) {
    if (!p || !info) return fail(GNNMP_EINVAL, "plan_info: null argument");
    info[0] = p->n_src;
    info[1] = p->n_dst;
    info[2] = p->n_edges;
    info[3] = p->n_total;
    info[4] = p->max_degree;
    info[5] = p->n_long;  // rows that are split
    info[6] = p->bytes;
    info[7] = p->long_thresh;
    return GNNMP_OK;
}

int gnnmp_plan_export(const gnnmp_graph_t *p, int32_t *rowptr, int32_t *col, int32_t *eid,
                      gnnmp_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!p) return fail(GNNMP_EINVAL, "plan_export: null plan");
    if (p->n_total > (int64_t)INT32_MAX)
        return fail(GNNMP_EUNSUPPORTED, "plan_export: E' = %lld does not fit int32 rowptr / eid (use gnnmp_plan_export64)",
                    (long long)p->n_total);
    if (rowptr)   // fewer than 2^31 slots: the unsigned values ARE the int32 values
        GNNMP_HIP(hipMemcpyAsync(rowptr, p->rowptr, sizeof(int32_t) * (size_t)(p->n_dst + 1), hipMemcpyDeviceToDevice, stream));
    if (col && p->n_total > 0)
        GNNMP_HIP(hipMemcpyAsync(col, p->col, sizeof(int32_t) * (size_t)p->n_total,
                                 hipMemcpyDeviceToDevice, stream));
    if (eid && p->n_total > 0)
        GNNMP_HIP(hipMemcpyAsync(eid, p->eid, sizeof(int32_t) * (size_t)p->n_total,
                                 hipMemcpyDeviceToDevice, stream));
    return GNNMP_OK;
}

int gnnmp_plan_export64(const gnnmp_graph_t *p, int64_t *rowptr, int32_t *col, uint32_t *eid, gnnmp_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!p) return fail(GNNMP_EINVAL, "plan_export64: null plan");
    if (rowptr) {
        widen_u32_kernel<<<nblocks(p->n_dst + 1, 256), 256, 0, stream>>>(p->rowptr, p->n_dst + 1, rowptr);
        GNNMP_LAUNCH_CHECK("widen_u32_kernel");
    }
    if (col && p->n_total > 0)
        GNNMP_HIP(hipMemcpyAsync(col, p->col, sizeof(int32_t) * (size_t)p->n_total, hipMemcpyDeviceToDevice, stream));
    if (eid && p->n_total > 0)
        GNNMP_HIP(hipMemcpyAsync(eid, p->eid, sizeof(uint32_t) * (size_t)p->n_total, hipMemcpyDeviceToDevice, stream));
    return GNNMP_OK;
}

int gnnmp_add_self_loops(const void *src, const void *dst, int idx_bytes, int index_base,
                         int64_t n_edges, int64_t n, void *out_src, void *out_dst, const float *w,
                         float *out_w, gnnmp_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (idx_bytes != 4 && idx_bytes != 8) return fail(GNNMP_EINVAL, "add_self_loops: idx_bytes %d", idx_bytes);
    if (index_base != 0 && index_base != 1) return fail(GNNMP_EINVAL, "add_self_loops: index_base %d", index_base);
    if (n_edges < 0 || n < 0) return fail(GNNMP_EINVAL, "add_self_loops: negative size");
    if ((w != nullptr && out_w == nullptr) || (w == nullptr && out_w != nullptr && n_edges > 0))
        return fail(GNNMP_EINVAL, "add_self_loops: w and out_w must both be NULL or both non-NULL");
    if (n_edges + n == 0) return GNNMP_OK;
    if (!out_src || !out_dst || (n_edges > 0 && (!src || !dst)))
        return fail(GNNMP_EINVAL, "add_self_loops: null pointer");
    self_loops_kernel<<<nblocks(n_edges + n, 256), 256, 0, stream>>>(
        src, dst, idx_bytes, index_base, n_edges, n, out_src, out_dst, w, out_w);
    GNNMP_LAUNCH_CHECK("self_loops_kernel");
    return GNNMP_OK;
}

int gnnmp_batch_coo(const void *src, const void *dst, int idx_bytes, int index_base,
                    const int64_t *edge_ptr, const int64_t *node_ptr, int64_t n_graphs,
                    void *out_src, void *out_dst, void *graph_indicator, gnnmp_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (idx_bytes != 4 && idx_bytes != 8) return fail(GNNMP_EINVAL, "batch_coo: idx_bytes %d", idx_bytes);
    if (index_base != 0 && index_base != 1) return fail(GNNMP_EINVAL, "batch_coo: index_base %d", index_base);
    if (n_graphs <= 0 || !edge_ptr || !node_ptr) return fail(GNNMP_EINVAL, "batch_coo: bad graph table");
    // totals live on the device; read them back (graph prep, not on the timed path)
    int64_t tot[2] = {0, 0};
    GNNMP_HIP(hipMemcpyAsync(&tot[0], edge_ptr + n_graphs, sizeof(int64_t), hipMemcpyDeviceToHost, stream));
    GNNMP_HIP(hipMemcpyAsync(&tot[1], node_ptr + n_graphs, sizeof(int64_t), hipMemcpyDeviceToHost, stream));
    GNNMP_HIP(hipStreamSynchronize(stream));
    if (tot[0] > 0) {
        if (!src || !dst || !out_src || !out_dst) return fail(GNNMP_EINVAL, "batch_coo: null edge arrays");
        batch_edges_kernel<<<nblocks(tot[0], 256), 256, 0, stream>>>(
            src, dst, idx_bytes, edge_ptr, node_ptr, n_graphs, tot[0], out_src, out_dst);
        GNNMP_LAUNCH_CHECK("batch_edges_kernel");
    }
    if (tot[1] > 0 && graph_indicator) {
        batch_indicator_kernel<<<nblocks(tot[1], 256), 256, 0, stream>>>(
            node_ptr, n_graphs, tot[1], idx_bytes, index_base, graph_indicator);
        GNNMP_LAUNCH_CHECK("batch_indicator_kernel");
    }
    return GNNMP_OK;
}

}  // extern "C"
