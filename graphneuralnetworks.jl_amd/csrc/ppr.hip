// ppr.hip — ppr_diffusion(g; alpha)      GNNGraphs/src/transform.jl:1026-1051      gnnmp_ppr_diffusion_f32
//   A = sparse(t, s, w, N, N) (parallel edges summed), M = I + (alpha32 - 1) * A, new_w[e] = alpha32 * inv(M)[t_e, s_e].
// The reference inverts the dense N x N matrix on the host.  A batched graph is block diagonal: every member graph of n nodes is its own
// n x n block, inverted IN PLACE (n * n floats; an augmented [M | I] would halve the graphs that fit in LDS) by Gauss-Jordan elimination
// with partial pivoting — one workgroup per member graph with the block in LDS (ppr_lds_kernel), or, for a graph whose block exceeds the
// LDS budget, the block in device scratch and two launches a pivot step (ppr_pivot_kernel: search, exchange, scale; ppr_update_kernel:
// the grid-wide rank-1 update), the pivot index and the singular mark staying on the device.
// Both paths call the SAME element operations (ppr_add_row, ppr_m_of, ppr_better, ppr_scale, ppr_update), each element sees them in the
// same order, and the pivot rule is an order-free maximum (largest |f_i|, lowest i on a tie): the two paths, a member graph alone and
// the same graph inside any batch give the same bits.  The step, with f_i = a_ik read for every row BEFORE anything moves:
//   p = the pivot row, piv = f_p; piv == 0: the block is singular, the step is skipped (uniformly: no lane leaves a barrier behind)
//   rows p and k are exchanged; r_j = (j == k ? 1 : a_kj) / piv
//   a_ij = fmaf(-f_i, r_j, j == k ? 0 : a_ij) for every i != k      (f_i of the row that came from k is the old a_kk)
// The exchanges are undone on the columns, last first, as an index map (src): Minv[i][j] = a[i][src[j]].
//
// LDS: a [n][n], f [n], the exchange list [n] (f is reused for src) — (n * n + 2 n) * 4 bytes: n <= 127 in the static 64 KB, n <= 201 in
// the 160 KB a launch may opt into.  A launch asks only for what its largest LDS-path graph needs (a ZINC-sized batch: ~5 KB), and takes
// 256 threads for blocks of up to 32 nodes, 1024 above.  Figures: DESIGN.md §3.
#include <cmath>
#include <vector>

#include "common.h"
#include "scratch.h"

namespace gnnmp {
namespace {

constexpr int PPR_BLOCK_SMALL = 256, PPR_BLOCK = 1024;
constexpr int PPR_SMALL_NODES = 32;               // member graphs up to here: PPR_BLOCK_SMALL threads a workgroup
constexpr int64_t PPR_LDS_DEFAULT = 64 * 1024;
constexpr int64_t PPR_LDS_MAX = 160 * 1024;
constexpr unsigned PPR_NOT_SINGULAR = 0xffffffffu;

inline unsigned nblk(int64_t n, int bs = 256) { return (unsigned)((n + bs - 1) / bs); }
inline int64_t lds_bytes_of(int64_t n) { return (n * n + 2 * n) * (int64_t)sizeof(float); }

struct PprRows {
    const uint32_t *rowptr;   // [N + 1] of the transposed plan
    const int32_t *col;       // per slot: the target t of the edge
    const int32_t *eid;       // per slot: original edge position (unsigned 32 bits)
    const float *w;           // [n_edges] or null
};

// ---- the element operations (both paths) -------------------------------------------------------------------------------------
// column s of A: the out-edges of node base + s in plan order, which is the original edge order; only this lane touches the column
__device__ __forceinline__ void ppr_add_row(const PprRows &r, int64_t base, int s, int n, float *a) {
    for (uint32_t x = r.rowptr[base + s], end = r.rowptr[base + s + 1]; x < end; ++x) {
        const int t = (int)((int64_t)r.col[x] - base);
        const float we = r.w ? r.w[(uint32_t)r.eid[x]] : 1.0f;
        a[(size_t)t * n + s] = a[(size_t)t * n + s] + we;
    }
}
__device__ __forceinline__ float ppr_m_of(float a, bool diag, float am1) { return (diag ? 1.0f : 0.0f) + am1 * a; }
// is (v, i) a better pivot than (bv, bi): larger magnitude, the lower row on a tie (a NaN is never better)
__device__ __forceinline__ bool ppr_better(float v, int i, float bv, int bi) { return v > bv || (v == bv && i < bi); }
__device__ __forceinline__ float ppr_scale(float a_pj, bool at_k, float piv) { return (at_k ? 1.0f : a_pj) / piv; }
__device__ __forceinline__ float ppr_update(float f_i, float r_j, float a_ij, bool at_k) { return fmaf(-f_i, r_j, at_k ? 0.0f : a_ij); }

__device__ __forceinline__ void ppr_wave_best(float &bv, int &bi) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const float ov = __shfl_xor(bv, d, 64);
        const int oi = __shfl_xor(bi, d, 64);
        if (ppr_better(ov, oi, bv, bi)) {
            bv = ov;
            bi = oi;
        }
    }
}

// the exchanges undone on the columns, last first: src[j] = the column of `a` that holds column j of the inverse (one lane, n steps)
__device__ __forceinline__ void ppr_unscramble(const int *perm, int *src, int n) {
    for (int k = n - 1; k >= 0; --k) {
        const int p = perm[k];
        if (p != k) {
            const int t = src[k];
            src[k] = src[p];
            src[p] = t;
        }
    }
}

// out[eid] = alpha * Minv[t][s] for the out-edges of node base + s
__device__ __forceinline__ void ppr_write_row(const PprRows &r, int64_t base, int s, int n, const float *a, const int *src, float alpha,
                                              float *out) {
    const int cs = src[s];
    for (uint32_t x = r.rowptr[base + s], end = r.rowptr[base + s + 1]; x < end; ++x) {
        const int t = (int)((int64_t)r.col[x] - base);
        out[(uint32_t)r.eid[x]] = alpha * a[(size_t)t * n + cs];
    }
}

__device__ __forceinline__ int64_t ppr_graph_bound(const void *graph_ptr, int idx_bytes, int64_t g, int64_t N) {
    return graph_ptr ? load_index(graph_ptr, g, idx_bytes, 0) : (g == 0 ? 0 : N);
}

// ---- LDS path: workgroup g inverts member graph g; graphs of more than max_nodes nodes belong to the scratch path ------------------
// Every barrier stands outside every condition that is not uniform over the workgroup: `ok` is computed by every wave from the same f.
__global__ void __launch_bounds__(PPR_BLOCK)
ppr_lds_kernel(const PprRows r, const void *graph_ptr, int idx_bytes, int64_t N, int64_t max_nodes, float alpha, float am1, float *out,
               unsigned *singular) {
    extern __shared__ float4 ppr_lds[];
    const int64_t base = ppr_graph_bound(graph_ptr, idx_bytes, blockIdx.x, N);
    const int64_t n64 = ppr_graph_bound(graph_ptr, idx_bytes, (int64_t)blockIdx.x + 1, N) - base;
    if (n64 > max_nodes || n64 <= 0) return;   // (the whole workgroup, before any barrier)
    const int n = (int)n64, nn = n * n;
    float *a = reinterpret_cast<float *>(ppr_lds);
    float *f = a + nn;
    int *perm = reinterpret_cast<int *>(f + n);
    const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63;
    // the walk of this lane over the elements x = i * n + j: x advances by nt, (i, j) by (di, dj) with one carry
    const int i0 = tid / n, j0 = tid % n, di = nt / n, dj = nt % n;

    for (int x = tid; x < nn; x += nt) a[x] = 0.0f;
    __syncthreads();
    for (int s = tid; s < n; s += nt) ppr_add_row(r, base, s, n, a);
    __syncthreads();
    for (int x = tid, i = i0, j = j0; x < nn; x += nt) {
        a[x] = ppr_m_of(a[x], i == j, am1);
        i += di;
        j += dj;
        if (j >= n) {
            j -= n;
            ++i;
        }
    }
    __syncthreads();

    for (int k = 0; k < n; ++k) {
        for (int i = tid; i < n; i += nt) f[i] = a[i * n + k];
        __syncthreads();
        float bv = -1.0f;
        int bi = 0x7fffffff;
        for (int i = k + lane; i < n; i += 64) {
            const float v = fabsf(f[i]);
            if (ppr_better(v, i, bv, bi)) {
                bv = v;
                bi = i;
            }
        }
        ppr_wave_best(bv, bi);
        const int p = bi == 0x7fffffff ? k : bi;   // (a column of NaN: no row is "better"; the NaN spreads, nothing hangs)
        const float piv = f[p];
        const bool ok = piv != 0.0f;
        if (ok) {
            for (int j = tid; j < n; j += nt) {
                const float vk = a[k * n + j], vp = a[p * n + j];
                if (p != k) a[p * n + j] = vk;
                a[k * n + j] = ppr_scale(vp, j == k, piv);
            }
        }
        if (tid == 0) {
            perm[k] = ok ? p : k;
            if (!ok) atomicMin(singular, (unsigned)blockIdx.x);
        }
        __syncthreads();
        if (ok) {
            const float fk = f[k];
            for (int x = tid, i = i0, j = j0; x < nn; x += nt) {
                if (i != k) a[x] = ppr_update(i == p ? fk : f[i], a[k * n + j], a[x], j == k);
                i += di;
                j += dj;
                if (j >= n) {
                    j -= n;
                    ++i;
                }
            }
        }
        __syncthreads();
    }

    int *src = reinterpret_cast<int *>(f);
    for (int j = tid; j < n; j += nt) src[j] = j;
    __syncthreads();
    if (tid == 0) ppr_unscramble(perm, src, n);
    __syncthreads();
    for (int s = tid; s < n; s += nt) ppr_write_row(r, base, s, n, a, src, alpha, out);
}

// ---- scratch path: one member graph at [base, base + n), a [n][n] in device memory -------------------------------------------------
__global__ void ppr_accum_kernel(const PprRows r, int64_t base, int n, float *a) {
    const int s = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (s < n) ppr_add_row(r, base, s, n, a);
}

// grid (columns / 256, n): row i = blockIdx.y
__global__ void ppr_m_kernel(float *a, int n, float am1) {
    const int i = (int)blockIdx.y, j = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (j < n) a[(size_t)i * n + j] = ppr_m_of(a[(size_t)i * n + j], i == j, am1);
}

// one workgroup: f = column k, the pivot search, the exchange and the scaling of step k.  info[0] = p, info[1] = 1 | 0 (step skipped)
__global__ void __launch_bounds__(PPR_BLOCK)
ppr_pivot_kernel(float *a, float *f, int n, int k, int *perm, int *info, unsigned *singular, unsigned member) {
    __shared__ float s_v[PPR_BLOCK / 64];
    __shared__ int s_i[PPR_BLOCK / 64];
    const int tid = threadIdx.x;
    float bv = -1.0f;
    int bi = 0x7fffffff;
    for (int i = tid; i < n; i += PPR_BLOCK) {
        const float fi = a[(size_t)i * n + k];
        f[i] = fi;
        const float v = fabsf(fi);
        if (i >= k && ppr_better(v, i, bv, bi)) {
            bv = v;
            bi = i;
        }
    }
    ppr_wave_best(bv, bi);
    if ((tid & 63) == 0) {
        s_v[tid >> 6] = bv;
        s_i[tid >> 6] = bi;
    }
    __syncthreads();
    bv = s_v[0];
    bi = s_i[0];
#pragma unroll
    for (int wv = 1; wv < PPR_BLOCK / 64; ++wv)
        if (ppr_better(s_v[wv], s_i[wv], bv, bi)) {
            bv = s_v[wv];
            bi = s_i[wv];
        }
    const int p = bi == 0x7fffffff ? k : bi;
    const float piv = a[(size_t)p * n + k];   // (nobody has written yet: the barrier below comes first)
    const bool ok = piv != 0.0f;
    __syncthreads();
    if (ok) {
        for (int j = tid; j < n; j += PPR_BLOCK) {
            const float vk = a[(size_t)k * n + j], vp = a[(size_t)p * n + j];
            if (p != k) a[(size_t)p * n + j] = vk;
            a[(size_t)k * n + j] = ppr_scale(vp, j == k, piv);
        }
    }
    if (tid == 0) {
        perm[k] = ok ? p : k;
        info[0] = p;
        info[1] = ok ? 1 : 0;
        if (!ok) atomicMin(singular, member);
    }
}

// grid (columns / 256, n): row i = blockIdx.y; row k (the scaled pivot row) is only read
__global__ void ppr_update_kernel(float *a, const float *f, int n, int k, const int *info) {
    const int i = (int)blockIdx.y, j = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (!info[1] || i == k || j >= n) return;
    const int p = info[0];
    a[(size_t)i * n + j] = ppr_update(i == p ? f[k] : f[i], a[(size_t)k * n + j], a[(size_t)i * n + j], j == k);
}

__global__ void ppr_unscramble_kernel(const int *perm, int *src, int n) {
    __shared__ int s_perm[GNNMP_PPR_MAX_NODES], s_src[GNNMP_PPR_MAX_NODES];
    for (int j = threadIdx.x; j < n; j += blockDim.x) {
        s_perm[j] = perm[j];
        s_src[j] = j;
    }
    __syncthreads();
    if (threadIdx.x == 0) ppr_unscramble(s_perm, s_src, n);
    __syncthreads();
    for (int j = threadIdx.x; j < n; j += blockDim.x) src[j] = s_src[j];
}

__global__ void ppr_write_kernel(const PprRows r, int64_t base, int n, const float *a, const int *src, float alpha, float *out) {
    const int s = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (s < n) ppr_write_row(r, base, s, n, a, src, alpha, out);
}

// ---- the check: graph_ptr ascends from 0 to N, and no edge leaves its graph's node range (as csrc/rwpe.hip checks it) ---------------
__global__ void ppr_check_ptr_kernel(const void *graph_ptr, int idx_bytes, int64_t G, int64_t N, int *bad) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k > G) return;
    const int64_t a = load_index(graph_ptr, k, idx_bytes, 0);
    if (k == 0 && a != 0) *bad = 1;
    if (k == G && a != N) *bad = 1;
    if (k < G && a > load_index(graph_ptr, k + 1, idx_bytes, 0)) *bad = 1;
}

// (reads graph_ptr[0 .. G] only, whatever it holds; the verdict counts only when ppr_check_ptr_kernel found nothing)
__global__ void ppr_check_edges_kernel(const PprRows r, const void *graph_ptr, int idx_bytes, int64_t G, int64_t N, int *bad) {
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

struct PprScratch {
    float *a, *f;
    int *perm, *src, *info;
};

// one member graph through device scratch: 2 n + 5 launches, no host synchronisation
int run_scratch(const PprRows &r, int64_t base, int n, unsigned member, const PprScratch &sc, float alpha, float am1, float *out,
                unsigned *singular, hipStream_t stream) {
    GNNMP_HIP(hipMemsetAsync(sc.a, 0, (size_t)n * n * sizeof(float), stream));
    ppr_accum_kernel<<<nblk(n), 256, 0, stream>>>(r, base, n, sc.a);
    GNNMP_LAUNCH_CHECK("ppr_accum_kernel");
    const dim3 grid(nblk(n), (unsigned)n);
    ppr_m_kernel<<<grid, 256, 0, stream>>>(sc.a, n, am1);
    GNNMP_LAUNCH_CHECK("ppr_m_kernel");
    for (int k = 0; k < n; ++k) {
        ppr_pivot_kernel<<<1, PPR_BLOCK, 0, stream>>>(sc.a, sc.f, n, k, sc.perm, sc.info, singular, member);
        GNNMP_LAUNCH_CHECK("ppr_pivot_kernel");
        ppr_update_kernel<<<grid, 256, 0, stream>>>(sc.a, sc.f, n, k, sc.info);
        GNNMP_LAUNCH_CHECK("ppr_update_kernel");
    }
    ppr_unscramble_kernel<<<1, 256, 0, stream>>>(sc.perm, sc.src, n);
    GNNMP_LAUNCH_CHECK("ppr_unscramble_kernel");
    ppr_write_kernel<<<nblk(n), 256, 0, stream>>>(r, base, n, sc.a, sc.src, alpha, out);
    GNNMP_LAUNCH_CHECK("ppr_write_kernel");
    return GNNMP_OK;
}

int too_large(int64_t member, int64_t n) {
    return fail(GNNMP_EUNSUPPORTED,
                "ppr_diffusion: member graph %lld has %lld nodes; the dense n x n block is supported up to GNNMP_PPR_MAX_NODES = %d nodes",
                (long long)member, (long long)n, GNNMP_PPR_MAX_NODES);
}

int ppr_diffusion(gnnmp_graph_t *plan_t, const gnnmp_ppr_t *job, hipStream_t stream) {
    if (!plan_t) return fail(GNNMP_EINVAL, "ppr_diffusion: null plan");
    if (!job) return fail(GNNMP_EINVAL, "ppr_diffusion: null job");
    const int idx_bytes = job->idx_bytes;
    if (idx_bytes != 4 && idx_bytes != 8) return fail(GNNMP_EINVAL, "ppr_diffusion: idx_bytes %d", idx_bytes);
    if (job->graph_ptr && job->n_graphs < 1) return fail(GNNMP_EINVAL, "ppr_diffusion: n_graphs %lld with a graph_ptr", (long long)job->n_graphs);
    if (!std::isfinite(job->alpha)) return fail(GNNMP_EINVAL, "ppr_diffusion: alpha is not finite");
    if (job->lds_budget_bytes < 0) return fail(GNNMP_EINVAL, "ppr_diffusion: negative lds_budget_bytes");
    // (the plan is read only from here on: a call refused above never touches it)
    const int64_t N = plan_t->n_dst, G = job->graph_ptr ? job->n_graphs : 1;
    if (plan_t->self_loops) return fail(GNNMP_EINVAL, "ppr_diffusion: the plan has added self loops");
    if (plan_t->n_src != plan_t->n_dst) return fail(GNNMP_EINVAL, "ppr_diffusion: the plan is not square (%lld x %lld)", (long long)plan_t->n_src, (long long)plan_t->n_dst);
    if (!job->out && plan_t->n_edges > 0) return fail(GNNMP_EINVAL, "ppr_diffusion: null out");
    if (G > 0x7fffffffLL) return fail(GNNMP_EUNSUPPORTED, "ppr_diffusion: %lld graphs", (long long)G);
    if (N == 0 || plan_t->n_edges == 0) return GNNMP_OK;
    if (!job->graph_ptr && N > GNNMP_PPR_MAX_NODES) return too_large(0, N);
    const int64_t budget = std::min(job->lds_budget_bytes == 0 ? PPR_LDS_DEFAULT : job->lds_budget_bytes, PPR_LDS_MAX);
    int64_t max_nodes = 0;   // graphs of at most this many nodes take the LDS path
    while (lds_bytes_of(max_nodes + 1) <= budget) ++max_nodes;
    const float alpha = job->alpha, am1 = alpha - 1.0f;

    PprRows r;
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
        ppr_check_ptr_kernel<<<nblk(G + 1), 256, 0, stream>>>(job->graph_ptr, idx_bytes, G, N, bad.get());
        GNNMP_LAUNCH_CHECK("ppr_check_ptr_kernel");
        ppr_check_edges_kernel<<<nblk(N), 256, 0, stream>>>(r, job->graph_ptr, idx_bytes, G, N, bad.get());
        GNNMP_LAUNCH_CHECK("ppr_check_edges_kernel");
        int hbad[2] = {0, 0};
        std::vector<unsigned char> raw((size_t)(G + 1) * idx_bytes);
        GNNMP_HIP(hipMemcpyAsync(hbad, bad.get(), 2 * sizeof(int), hipMemcpyDeviceToHost, stream));
        GNNMP_HIP(hipMemcpyAsync(raw.data(), job->graph_ptr, raw.size(), hipMemcpyDeviceToHost, stream));
        GNNMP_HIP(hipStreamSynchronize(stream));
        if (hbad[0]) return fail(GNNMP_EINVAL, "ppr_diffusion: graph_ptr does not ascend from 0 to the %lld nodes", (long long)N);
        if (hbad[1]) return fail(GNNMP_EINVAL, "ppr_diffusion: an edge leaves its graph's node range");
        ptr.resize((size_t)G + 1);
        for (int64_t k = 0; k <= G; ++k)
            ptr[k] = idx_bytes == 8 ? reinterpret_cast<const int64_t *>(raw.data())[k] : (int64_t)reinterpret_cast<const int32_t *>(raw.data())[k];
    }

    int64_t lds_nodes = 0, large_nodes = 0;   // the largest graph of the LDS path and of the scratch path
    for (int64_t k = 0; k < G; ++k) {
        const int64_t n = ptr[k + 1] - ptr[k];
        if (n > GNNMP_PPR_MAX_NODES) return too_large(k, n);
        if (n > max_nodes)
            large_nodes = std::max(large_nodes, n);
        else
            lds_nodes = std::max(lds_nodes, n);
    }

    // (the buffers are hipFree'd when the call returns: that waits for the launches that use them)
    DevBuf<unsigned> singular;
    DevBuf<float> mat;
    DevBuf<int> ints;
    GNNMP_HIP(singular.alloc(1));
    GNNMP_HIP(hipMemsetAsync(singular.get(), 0xff, sizeof(unsigned), stream));
    if (lds_nodes > 0) {
        const size_t lds_bytes = (size_t)lds_bytes_of(lds_nodes);
        if (lds_bytes > 64 * 1024) GNNMP_LDS_OPTIN("ppr_lds_kernel", &ppr_lds_kernel);
        const int block = lds_nodes <= PPR_SMALL_NODES ? PPR_BLOCK_SMALL : PPR_BLOCK;
        ppr_lds_kernel<<<(unsigned)G, block, lds_bytes, stream>>>(r, job->graph_ptr, idx_bytes, N, max_nodes, alpha, am1, job->out, singular.get());
        GNNMP_LAUNCH_CHECK("ppr_lds_kernel");
    }
    if (large_nodes > 0) {
        GNNMP_HIP(mat.alloc((size_t)(large_nodes * large_nodes + large_nodes)));
        GNNMP_HIP(ints.alloc((size_t)(2 * large_nodes + 2)));
        PprScratch sc;
        sc.a = mat.get();
        sc.f = sc.a + large_nodes * large_nodes;
        sc.perm = ints.get();
        sc.src = sc.perm + large_nodes;
        sc.info = sc.src + large_nodes;
        for (int64_t k = 0; k < G; ++k)
            if (ptr[k + 1] - ptr[k] > max_nodes)
                GNNMP_TRY(run_scratch(r, ptr[k], (int)(ptr[k + 1] - ptr[k]), (unsigned)k, sc, alpha, am1, job->out, singular.get(), stream));
    }
    unsigned first = PPR_NOT_SINGULAR;
    GNNMP_HIP(hipMemcpyAsync(&first, singular.get(), sizeof(unsigned), hipMemcpyDeviceToHost, stream));
    GNNMP_HIP(hipStreamSynchronize(stream));
    if (first != PPR_NOT_SINGULAR)
        return fail(GNNMP_EINVAL, "ppr_diffusion: member graph %u is singular (I + (alpha - 1) A has an exactly zero pivot)", first);
    return GNNMP_OK;
}

}  // namespace
}  // namespace gnnmp

using namespace gnnmp;

extern "C" {

int gnnmp_ppr_diffusion_f32(gnnmp_graph_t *plan_t, const gnnmp_ppr_t *job, gnnmp_stream_t stream) {
    return ppr_diffusion(plan_t, job, (hipStream_t)stream);
}

}  // extern "C"
