// rwpe.hip — random_walk_pe(g, walk_length)      GNNGraphs/src/transform.jl:975-990      gnnmp_random_walk_pe_f32
//   A = adjacency_matrix(g, Float32; dir = :out), deg = row sums, dinv = 1 ./ deg with Inf -> 0, RW = A * Diagonal(dinv) (the COLUMN is
//   scaled, by the target's out-degree), pe[k, c] = (RW^k)[c, c].
// The reference multiplies N x N matrices and keeps their diagonals.  Here column c of RW^k is k propagates of the unit vector e_c over
// the TRANSPOSED plan (row i = the out-edges of i, in original edge order):
//   v_k[i] = sum over the edges e: i -> j, in plan order, of (w_e * dinv[j]) * v_{k-1}[j],      pe[k, c] = v_k[c]
// and a batched graph is block diagonal, so a tile of RWPE_T start nodes of one member graph needs two [n_g][RWPE_T] panels and nothing
// else: they live in LDS (rwpe_graph_kernel), or in device scratch for a graph whose panels exceed the LDS budget (rwpe_panel_kernel).
// Both kernels call ONE row walk (rwpe_walk_row) and one degree fold (rwpe_row_dinv): every sum runs in plan order in fp32 without
// contraction, so the two paths, any tiling and any batching give the same bits.  No atomics.
//
// The figures: RWPE_T = 16 columns are 64 bytes of a panel row, read as one ds_read_b128 by each of the 4 lanes of a
// row's lane group (consecutive columns in consecutive lanes; a wave covers 16 rows).  The default LDS budget is 64 KB a workgroup —
// the static limit, so no opt-in is needed, and 160 KB / 64 KB leaves two workgroups resident per CU; at (2 T + 1) floats a node it holds
// graphs of up to 496 nodes.  A launch asks only for what its largest LDS-path graph needs (a ZINC-sized batch: ~5 KB).
#include <vector>

#include "common.h"
#include "scratch.h"

namespace gnnmp {
namespace {

constexpr int RWPE_T = GNNMP_RWPE_TILE;           // start nodes (panel columns) per tile
constexpr int RWPE_VEC = 4;                       // columns per lane: one 16-byte panel access
constexpr int RWPE_LPG = RWPE_T / RWPE_VEC;       // lanes per row
constexpr int RWPE_BLOCK = 256;
constexpr int RWPE_RPB = RWPE_BLOCK / RWPE_LPG;   // rows per pass of a workgroup
constexpr int64_t RWPE_LDS_DEFAULT = 64 * 1024;
constexpr int64_t RWPE_LDS_MAX = 160 * 1024;
constexpr int64_t RWPE_NODE_BYTES = (2 * RWPE_T + 1) * (int64_t)sizeof(float);   // two panel rows and dinv
constexpr int64_t RWPE_PANEL_BATCH_BYTES = (int64_t)64 << 20;                    // scratch panels of one batch of tiles (global path)
static_assert(RWPE_T % RWPE_VEC == 0 && RWPE_BLOCK % RWPE_LPG == 0, "a lane group covers the tile");

inline unsigned nblk(int64_t n, int bs = 256) { return (unsigned)((n + bs - 1) / bs); }

struct RwpeRows {
    const uint32_t *rowptr;   // [N + 1] of the transposed plan
    const int32_t *col;       // per slot: the target j of the edge
    const int32_t *eid;       // per slot: original edge position (unsigned 32 bits)
    const float *w;           // [n_edges] or null
};

// dinv of node `row`: 1 / (the sum of its out-edge weights in plan order; 1 per edge without weights), Inf -> 0
__device__ __forceinline__ float rwpe_row_dinv(const RwpeRows &r, int64_t row) {
    float deg = 0.0f;
    for (uint32_t s = r.rowptr[row], end = r.rowptr[row + 1]; s < end; ++s) deg += r.w ? r.w[(uint32_t)r.eid[s]] : 1.0f;
    const float inv = 1.0f / deg;
    return __builtin_isinf(inv) ? 0.0f : inv;
}

// THE row walk: acc[0 .. 3] = columns 4 q .. 4 q + 3 of row `row` of the next panel.  dinv and cur are the graph's own (indexed by
// node - base), in LDS or in device memory.
__device__ __forceinline__ void rwpe_walk_row(const RwpeRows &r, int64_t base, int64_t row, int q, const float *dinv, const float *cur,
                                              float acc[RWPE_VEC]) {
#pragma unroll
    for (int c = 0; c < RWPE_VEC; ++c) acc[c] = 0.0f;
    for (uint32_t s = r.rowptr[row], end = r.rowptr[row + 1]; s < end; ++s) {
        const int64_t j = (int64_t)r.col[s] - base;
        const float we = r.w ? r.w[(uint32_t)r.eid[s]] : 1.0f;
        const float coef = we * dinv[j];
        const float4 v = *reinterpret_cast<const float4 *>(cur + j * RWPE_T + q * RWPE_VEC);
        acc[0] += coef * v.x;
        acc[1] += coef * v.y;
        acc[2] += coef * v.z;
        acc[3] += coef * v.w;
    }
}

// the lane that holds column c = i - c0 of row i owns out[base + i][k]
__device__ __forceinline__ void rwpe_store_diag(float *out, int64_t node, int64_t K, int64_t k, int64_t c, int q, const float acc[RWPE_VEC]) {
    if (c < (int64_t)q * RWPE_VEC || c >= (int64_t)(q + 1) * RWPE_VEC) return;
    const int cc = (int)(c - (int64_t)q * RWPE_VEC);
    out[node * K + k] = cc == 0 ? acc[0] : cc == 1 ? acc[1] : cc == 2 ? acc[2] : acc[3];
}

__device__ __forceinline__ int64_t rwpe_graph_bound(const void *graph_ptr, int idx_bytes, int64_t g, int64_t N) {
    return graph_ptr ? load_index(graph_ptr, g, idx_bytes, 0) : (g == 0 ? 0 : N);
}

// LDS path.  Block (g, ty): the start nodes c0 .. c0 + T of graph g, c0 = ty * T; graphs of more than max_nodes nodes belong to the
// global path.  LDS: cur [n][T], next [n][T], dinv [n].
__global__ void __launch_bounds__(RWPE_BLOCK)
rwpe_graph_kernel(const RwpeRows r, const void *graph_ptr, int idx_bytes, int64_t N, int64_t max_nodes, int64_t K, float *out) {
    extern __shared__ float4 rwpe_lds[];
    const int64_t base = rwpe_graph_bound(graph_ptr, idx_bytes, blockIdx.x, N);
    const int n = (int)(rwpe_graph_bound(graph_ptr, idx_bytes, (int64_t)blockIdx.x + 1, N) - base);
    const int c0 = (int)blockIdx.y * RWPE_T;
    if ((int64_t)n > max_nodes || c0 >= n) return;
    float *cur = reinterpret_cast<float *>(rwpe_lds);
    float *nxt = cur + n * RWPE_T;
    float *dinv = nxt + n * RWPE_T;
    const int tid = threadIdx.x;
    for (int i = tid; i < n; i += RWPE_BLOCK) dinv[i] = rwpe_row_dinv(r, base + i);
    for (int x = tid; x < n * RWPE_T; x += RWPE_BLOCK) cur[x] = (x / RWPE_T == c0 + x % RWPE_T) ? 1.0f : 0.0f;
    __syncthreads();
    const int q = tid % RWPE_LPG;
    for (int64_t k = 0; k < K; ++k) {
        for (int i = tid / RWPE_LPG; i < n; i += RWPE_RPB) {
            float acc[RWPE_VEC];
            rwpe_walk_row(r, base, base + i, q, dinv, cur, acc);
            *reinterpret_cast<float4 *>(nxt + i * RWPE_T + q * RWPE_VEC) = make_float4(acc[0], acc[1], acc[2], acc[3]);
            rwpe_store_diag(out, base + i, K, k, (int64_t)i - c0, q, acc);
        }
        __syncthreads();   // next is complete, and nobody reads cur any more: it is the next step's target
        float *t = cur;
        cur = nxt;
        nxt = t;
    }
}

// ---- global path -----------------------------------------------------------------------------------------------------------
__global__ void rwpe_dinv_kernel(const RwpeRows r, int64_t N, float *dinv) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < N) dinv[i] = rwpe_row_dinv(r, i);
}

// panels: [tiles of the batch][2][n][T]; tile blockIdx.y starts at c0 = (tile0 + blockIdx.y) * T
__global__ void rwpe_panel_init_kernel(float *panels, int64_t n, int64_t tile0) {
    const int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= n * RWPE_T) return;
    const int64_t c0 = (tile0 + blockIdx.y) * RWPE_T;
    panels[(int64_t)blockIdx.y * 2 * n * RWPE_T + x] = (x / RWPE_T == c0 + x % RWPE_T) ? 1.0f : 0.0f;
}

// one step of one batch of tiles of the graph at [base, base + n): step k reads panel k & 1 and writes the other
__global__ void __launch_bounds__(RWPE_BLOCK)
rwpe_panel_kernel(const RwpeRows r, int64_t base, int64_t n, int64_t tile0, const float *dinv, float *panels, int64_t K, int64_t k,
                  float *out) {
    const int64_t i = ((int64_t)blockIdx.x * RWPE_BLOCK + threadIdx.x) / RWPE_LPG;
    if (i >= n) return;
    const int q = threadIdx.x % RWPE_LPG;
    const int64_t c0 = (tile0 + blockIdx.y) * RWPE_T;
    float *p0 = panels + (int64_t)blockIdx.y * 2 * n * RWPE_T;
    const float *cur = p0 + (k & 1) * n * RWPE_T;
    float *nxt = p0 + ((k & 1) ^ 1) * n * RWPE_T;
    float acc[RWPE_VEC];
    rwpe_walk_row(r, base, base + i, q, dinv + base, cur, acc);
    *reinterpret_cast<float4 *>(nxt + i * RWPE_T + q * RWPE_VEC) = make_float4(acc[0], acc[1], acc[2], acc[3]);
    rwpe_store_diag(out, base + i, K, k, i - c0, q, acc);
}

// ---- the check: graph_ptr ascends from 0 to N, and no edge leaves its graph's node range -------------------------------------
__global__ void rwpe_check_ptr_kernel(const void *graph_ptr, int idx_bytes, int64_t G, int64_t N, int *bad) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k > G) return;
    const int64_t a = load_index(graph_ptr, k, idx_bytes, 0);
    if (k == 0 && a != 0) *bad = 1;
    if (k == G && a != N) *bad = 1;
    if (k < G && a > load_index(graph_ptr, k + 1, idx_bytes, 0)) *bad = 1;
}

// (reads graph_ptr[0 .. G] only, whatever it holds; the verdict counts only when rwpe_check_ptr_kernel found nothing)
__global__ void rwpe_check_edges_kernel(const RwpeRows r, const void *graph_ptr, int idx_bytes, int64_t G, int64_t N, int *bad) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    int64_t lo = 0, hi = G;   // the last graph in [0, G) that starts at or before i
    while (hi - lo > 1) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (load_index(graph_ptr, mid, idx_bytes, 0) <= i)
            lo = mid;
        else
            hi = mid;
    }
    const int64_t a = load_index(graph_ptr, lo, idx_bytes, 0), b = load_index(graph_ptr, lo + 1, idx_bytes, 0);
    if (i < a || i >= b) {
        bad[1] = 1;
        return;
    }
    for (uint32_t s = r.rowptr[i], end = r.rowptr[i + 1]; s < end; ++s) {
        const int64_t j = r.col[s];
        if (j < a || j >= b) bad[1] = 1;
    }
}

// one graph through device scratch (panels: room for `batch` tiles): an init launch and K step launches per batch of tiles
int run_panels(const RwpeRows &r, int64_t base, int64_t n, const float *dinv, float *panels, int64_t batch, int64_t K, float *out,
               hipStream_t stream) {
    const int64_t tiles = (n + RWPE_T - 1) / RWPE_T;
    for (int64_t tile0 = 0; tile0 < tiles; tile0 += batch) {
        const unsigned nb = (unsigned)std::min<int64_t>(batch, tiles - tile0);
        rwpe_panel_init_kernel<<<dim3(nblk(n * RWPE_T), nb), 256, 0, stream>>>(panels, n, tile0);
        GNNMP_LAUNCH_CHECK("rwpe_panel_init_kernel");
        for (int64_t k = 0; k < K; ++k) {
            rwpe_panel_kernel<<<dim3(nblk(n * RWPE_LPG, RWPE_BLOCK), nb), RWPE_BLOCK, 0, stream>>>(r, base, n, tile0, dinv, panels, K, k, out);
            GNNMP_LAUNCH_CHECK("rwpe_panel_kernel");
        }
    }
    return GNNMP_OK;
}

int random_walk_pe(gnnmp_graph_t *plan_t, const gnnmp_rwpe_t *job, int64_t lds_budget, hipStream_t stream) {
    if (!plan_t) return fail(GNNMP_EINVAL, "random_walk_pe: null plan");
    if (!job) return fail(GNNMP_EINVAL, "random_walk_pe: null job");
    if (!job->out) return fail(GNNMP_EINVAL, "random_walk_pe: null out");
    const int64_t K = job->walk_length, G = job->graph_ptr ? job->n_graphs : 1;
    const int idx_bytes = job->idx_bytes;
    if (K < 1 || K > GNNMP_RWPE_MAX_WALK) return fail(GNNMP_EINVAL, "random_walk_pe: walk_length %lld outside 1 .. %d", (long long)K, GNNMP_RWPE_MAX_WALK);
    if (idx_bytes != 4 && idx_bytes != 8) return fail(GNNMP_EINVAL, "random_walk_pe: idx_bytes %d", idx_bytes);
    if (job->graph_ptr && job->n_graphs < 1) return fail(GNNMP_EINVAL, "random_walk_pe: n_graphs %lld with a graph_ptr", (long long)job->n_graphs);
    if (lds_budget < 0) return fail(GNNMP_EINVAL, "random_walk_pe: negative lds_budget_bytes");
    // (the plan is read only from here on: a call refused above never touches it)
    const int64_t N = plan_t->n_dst;
    if (plan_t->self_loops) return fail(GNNMP_EINVAL, "random_walk_pe: the plan has added self loops");
    if (plan_t->n_src != plan_t->n_dst) return fail(GNNMP_EINVAL, "random_walk_pe: the plan is not square (%lld x %lld)", (long long)plan_t->n_src, (long long)plan_t->n_dst);
    if (G > 0x7fffffffLL) return fail(GNNMP_EUNSUPPORTED, "random_walk_pe: %lld graphs", (long long)G);
    if (N == 0 && !job->graph_ptr) return GNNMP_OK;
    const int64_t budget = std::min(lds_budget == 0 ? RWPE_LDS_DEFAULT : lds_budget, RWPE_LDS_MAX);
    const int64_t max_nodes = budget / RWPE_NODE_BYTES;   // graphs of at most this many nodes take the LDS path

    RwpeRows r;
    r.rowptr = plan_t->rowptr;
    r.col = plan_t->col;
    r.eid = plan_t->eid;
    r.w = job->w;

    // node offsets on the host: [0, N] for one graph
    std::vector<int64_t> ptr{0, N};
    if (job->graph_ptr) {
        DevBuf<int> bad;   // [0] graph_ptr, [1] an edge
        GNNMP_HIP(bad.alloc(2));
        GNNMP_HIP(hipMemsetAsync(bad.get(), 0, 2 * sizeof(int), stream));
        rwpe_check_ptr_kernel<<<nblk(G + 1), 256, 0, stream>>>(job->graph_ptr, idx_bytes, G, N, bad.get());
        GNNMP_LAUNCH_CHECK("rwpe_check_ptr_kernel");
        if (N > 0) {
            rwpe_check_edges_kernel<<<nblk(N), 256, 0, stream>>>(r, job->graph_ptr, idx_bytes, G, N, bad.get());
            GNNMP_LAUNCH_CHECK("rwpe_check_edges_kernel");
        }
        int hbad[2] = {0, 0};
        std::vector<unsigned char> raw((size_t)(G + 1) * idx_bytes);
        GNNMP_HIP(hipMemcpyAsync(hbad, bad.get(), 2 * sizeof(int), hipMemcpyDeviceToHost, stream));
        GNNMP_HIP(hipMemcpyAsync(raw.data(), job->graph_ptr, raw.size(), hipMemcpyDeviceToHost, stream));
        GNNMP_HIP(hipStreamSynchronize(stream));
        if (hbad[0]) return fail(GNNMP_EINVAL, "random_walk_pe: graph_ptr does not ascend from 0 to the %lld nodes", (long long)N);
        if (hbad[1]) return fail(GNNMP_EINVAL, "random_walk_pe: an edge leaves its graph's node range");
        ptr.resize((size_t)G + 1);
        for (int64_t k = 0; k <= G; ++k)
            ptr[k] = idx_bytes == 8 ? reinterpret_cast<const int64_t *>(raw.data())[k] : (int64_t)reinterpret_cast<const int32_t *>(raw.data())[k];
    }
    if (N == 0) return GNNMP_OK;

    int64_t lds_nodes = 0, large_nodes = 0;   // the largest graph of the LDS path and of the global path
    for (int64_t k = 0; k < G; ++k) {
        const int64_t n = ptr[k + 1] - ptr[k];
        if (n > max_nodes)
            large_nodes = std::max(large_nodes, n);
        else
            lds_nodes = std::max(lds_nodes, n);
    }
    if (lds_nodes > 0) {
        const size_t lds_bytes = (size_t)(lds_nodes * RWPE_NODE_BYTES);
        if (lds_bytes > 64 * 1024) GNNMP_LDS_OPTIN("rwpe_graph_kernel", &rwpe_graph_kernel);
        const dim3 grid((unsigned)G, (unsigned)((lds_nodes + RWPE_T - 1) / RWPE_T));
        rwpe_graph_kernel<<<grid, RWPE_BLOCK, lds_bytes, stream>>>(r, job->graph_ptr, idx_bytes, N, max_nodes, K, job->out);
        GNNMP_LAUNCH_CHECK("rwpe_graph_kernel");
    }
    if (large_nodes > 0) {
        // (both buffers are hipFree'd when the call returns: that waits for the launches that use them)
        const int64_t tile_floats = 2 * large_nodes * RWPE_T;
        const int64_t batch = std::max<int64_t>(1, std::min<int64_t>({(large_nodes + RWPE_T - 1) / RWPE_T,
                                                                      RWPE_PANEL_BATCH_BYTES / (tile_floats * (int64_t)sizeof(float)), (int64_t)65535}));
        DevBuf<float> dinv, panels;
        GNNMP_HIP(dinv.alloc((size_t)N));
        GNNMP_HIP(panels.alloc((size_t)(batch * tile_floats)));
        rwpe_dinv_kernel<<<nblk(N), 256, 0, stream>>>(r, N, dinv.get());
        GNNMP_LAUNCH_CHECK("rwpe_dinv_kernel");
        for (int64_t k = 0; k < G; ++k)
            if (ptr[k + 1] - ptr[k] > max_nodes)
                GNNMP_TRY(run_panels(r, ptr[k], ptr[k + 1] - ptr[k], dinv.get(), panels.get(), batch, K, job->out, stream));
        GNNMP_HIP(hipStreamSynchronize(stream));
        return GNNMP_OK;
    }
    GNNMP_HIP(hipStreamSynchronize(stream));
    return GNNMP_OK;
}

}  // namespace
}  // namespace gnnmp

using namespace gnnmp;

extern "C" {

int gnnmp_random_walk_pe_f32(gnnmp_graph_t *plan_t, const gnnmp_rwpe_t *job, gnnmp_stream_t stream) {
    return random_walk_pe(plan_t, job, 0, (hipStream_t)stream);
}

int gnnmp_debug_random_walk_pe_f32(gnnmp_graph_t *plan_t, const gnnmp_rwpe_t *job, int64_t lds_budget_bytes, gnnmp_stream_t stream) {
    return random_walk_pe(plan_t, job, lds_budget_bytes, (hipStream_t)stream);
}

}  // extern "C"
