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
__device__ __forceinline__ void topk_emit(const TopkArgs &a, int64_t i, int64_t n, uint32_t gt, uint32_t eqb) {
    int64_t kg = a.k;
    if (a.k == 0) kg = (int64_t)ceil(a.ratio * (double)n);
    if (kg > n) kg = n;
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
