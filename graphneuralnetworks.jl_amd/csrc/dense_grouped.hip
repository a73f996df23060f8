// dense_grouped.hip — the dense contraction with ONE WEIGHT PER ROW SEGMENT, forward and adjoints (gnnmp.h):
//   out[n][:] = act(W_g x[n][:] + b_g)   for the rows n of group g, seg_ptr[g] <= n < seg_ptr[g + 1]
//   dW[g][o][k] = Σ_{n in g} dz[n][o] x[n][k],   db[g][o] = Σ_{n in g} dz[n][o]
// (Δx is the forward with the weight read transposed, as for gnnmp_dense_f32.)  Per-snapshot weights (EvolveGCNO), per-member-graph or
// per-node-type linear maps: what a host loop of gnnmp_dense_f32 / gnnmp_dense_grad_w_f32 spends one launch a group on.
// The boundaries are a device array and are never brought to the host: dense_grouped_route.h plans every launch from N, G, K, Dout.
//
// grouped_t16_kernel   the fp32 v_mfma_f32_16x16x4_f32 core of mfma16.h (operand image of W in LDS, x rows straight from HBM into the B
//                      operands, one 16-byte store per accumulator).  What is new is the split of the work: the row space is cut into
//                      SUPER-TILES of waves x 16 rows whatever the groups are, a persistent block owns a contiguous range of them and keeps
//                      the image and bias of ONE group resident.  It finds the group of its first row by a binary search of seg_ptr and
//                      then walks seg_ptr forward: per group that meets its range one image fill between two barriers, then the
//                      super-tiles the group meets, each wave its 16 rows.  Rows of a tile that belong to another group are zeros at the
//                      load and skipped at the store — a super-tile cut by boundaries is walked once per group it meets, every row is
//                      written exactly once.  No tile list, no prefix array, no scratch; empty groups are stepped over.
// grouped_fma_kernel   every other shape (any K, any Dout, any 4-byte alignment): lanes over the output columns of a block's rows, a
//                      k-ordered fmaf chain, the group of a row found the same way.
// grouped_gradw16_kernel / grouped_gradw_fma_kernel   block b reduces slab b % S of group b / S — the slab's bounds come from seg_ptr on
//                      the device — into a private partial; grouped_fold_kernel adds a group's S partials in slab order.  No atomics.
#include <algorithm>

#include "dense_grouped_route.h"
#include "launch.h"
#include "mfma16.h"

namespace gnnmp {

struct GroupedArgs {
    const float *x;
    int64_t ldx;
    const float *W;
    int64_t w_stride, sj, sk;   // W_g(j, k) at W[g * w_stride + j * sj + k * sk]
    const float *bias;
    int64_t bias_stride;
    const int64_t *seg_ptr;
    int64_t G;
    int act;
    float *out;
    int64_t ldo;
    int64_t N;
    int K, Dout;
    int waves;
    int64_t per_block;          // t16: super-tiles a block; fma: rows a block
};

// the first group g of [0, G) whose end lies past row r (G - 1 if there is none): the group of r when seg_ptr keeps its contract
__device__ __forceinline__ int64_t grouped_find(const int64_t *__restrict__ seg_ptr, int64_t G, int64_t r) {
    int64_t lo = 0, hi = G - 1;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (seg_ptr[mid + 1] > r) hi = mid; else lo = mid + 1;
    }
    return lo;
}

template <int NCB>
__global__ void __launch_bounds__(t16_max_threads(NCB)) grouped_t16_kernel(const GroupedArgs a) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    constexpr int DP = NCB * 16;
    f32x4 *img = reinterpret_cast<f32x4 *>(lds_raw);
    const int tid = threadIdx.x, nthreads = a.waves * 64;
    const int n0 = (int)blockIdx.y * DP;
    const int ncols = min(DP, a.Dout - n0);
    f32x4 *bias4 = img + t16_img_rows(a.K) * DP;
    const int lane = tid & 63, wave = tid >> 6;
    const int n = lane & 15, q = lane >> 4;
    const int64_t SR = (int64_t)a.waves * 16;                         // rows of a super-tile
    const int64_t row_lo = (int64_t)blockIdx.x * a.per_block * SR;
    const int64_t row_hi = min(a.N, row_lo + a.per_block * SR);
    if (row_lo >= row_hi) return;
    const bool has_bias = a.bias != nullptr;
    // everything that steers the loop below comes from blockIdx and seg_ptr: the same in every thread, the barriers are met by all
    for (int64_t g = grouped_find(a.seg_ptr, a.G, row_lo); g < a.G; ++g) {
        const int64_t gs = a.seg_ptr[g], ge = a.seg_ptr[g + 1];
        if (gs >= row_hi) break;
        const int64_t lo = max(gs, row_lo), hi = min(ge, row_hi);      // the group's rows in this block's range
        if (lo >= hi) continue;                                        // an empty group
        __syncthreads();                                               // the previous group's last reads of the image
        t16_fill_image(img, 0, DP, a.W + g * a.w_stride, a.sj, a.sk, a.K, n0, ncols, tid, nthreads);
        for (int i = tid; i < DP / 4; i += nthreads) {
            f32x4 b = {0.0f, 0.0f, 0.0f, 0.0f};
            if (has_bias) {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (4 * i + r < ncols) b[r] = a.bias[g * a.bias_stride + n0 + 4 * i + r];
            }
            bias4[i] = b;
        }
        __syncthreads();
        for (int64_t t0 = (lo / SR) * SR + wave * 16; t0 < hi; t0 += SR) {
            if (t0 + 16 <= lo) continue;                               // this wave's tile lies before the group
            const int64_t row = t0 + n;
            const bool ok = row >= lo && row < hi;
            const float *xr = a.x + min(max(row, lo), hi - 1) * a.ldx;
            f32x4 acc[NCB];
#pragma unroll
            for (int c = 0; c < NCB; ++c) acc[c] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            t16_segment_rt<NCB>(acc, img, 0, a.K >> 2, n, q, [&](int kcol) {
                const float4 v = *reinterpret_cast<const float4 *>(xr + kcol);
                return ok ? v : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            });
            t16_store<NCB>(acc, bias4, has_bias, a.act, a.out + row * a.ldo + n0, ok, ncols, q);
        }
    }
}

__global__ void __launch_bounds__(256) grouped_fma_kernel(const GroupedArgs a) {
    const int64_t row_lo = (int64_t)blockIdx.x * a.per_block;
    const int64_t row_hi = min(a.N, row_lo + a.per_block);
    if (row_lo >= row_hi) return;
    int64_t g = grouped_find(a.seg_ptr, a.G, row_lo);
    const int64_t items = (row_hi - row_lo) * a.Dout;
    for (int64_t idx = threadIdx.x; idx < items; idx += 256) {        // a thread's rows ascend: its group only moves forward
        const int64_t r = row_lo + idx / a.Dout;
        const int c = (int)(idx % a.Dout);
        while (g + 1 < a.G && a.seg_ptr[g + 1] <= r) ++g;
        const float *xr = a.x + r * a.ldx;
        const float *w = a.W + g * a.w_stride + c * a.sj;
        float acc = 0.0f;
        for (int k = 0; k < a.K; ++k) acc = fmaf(xr[k], w[k * a.sk], acc);
        if (a.bias) acc = acc + a.bias[g * a.bias_stride + c];
        if (a.act == GNNMP_ACT_RELU) acc = acc < 0.0f ? 0.0f : acc;   // NNlib.relu (NaN-preserving)
        a.out[r * a.ldo + c] = acc;
    }
}

// ---- the weight gradient ----------------------------------------------------------------------------------------------------------------
struct GroupedGradArgs {
    const float *dz;
    int64_t lddz;
    const float *x;
    int64_t ldx;
    const int64_t *seg_ptr;
    int64_t N, G;
    int S;
    float *part_w;     // [G * S][Dout * K], or null
    float *part_b;     // [G * S][Dout], or null
    int Dout, K;
    int tiles_per_wave;
};

// rows [n0, n1) of slab b % S of group b / S: the group's rows cut into S runs of a multiple of four rows (the four rows of an MFMA step
// never straddle slabs); bounds outside [0, N] — a seg_ptr that broke its contract — are clamped, nothing outside x and dz is read
__device__ __forceinline__ void grouped_slab(const GroupedGradArgs &a, int64_t b, int64_t &n0, int64_t &n1) {
    const int64_t g = b / a.S, s = b - g * a.S;
    const int64_t gs = min(max(a.seg_ptr[g], (int64_t)0), a.N), ge = min(max(a.seg_ptr[g + 1], gs), a.N);
    const int64_t rps = (((ge - gs) + a.S - 1) / a.S + 3) & ~(int64_t)3;
    n0 = min(ge, gs + s * rps);
    n1 = min(ge, n0 + rps);
}

// The tile split of dense_gradw16_kernel (dense_backward.hip): lane (i, q) supplies dz[n + q][o0 + 16 t + i] and x[n + q][k0 + 16 u + i] of a
// batch of four rows, both straight from the row-major matrices; a wave owns up to TO x TK tiles of 16 x 16, the waves of a block share
// the dz rows and split the columns of dW.  The next batch's loads are issued before the current batch's MFMAs.
template <int TO, int TK>
__global__ void __launch_bounds__(256) grouped_gradw16_kernel(const GroupedGradArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = lane & 15, q = lane >> 4;
    const int o0 = (int)blockIdx.y * 128;
    const int k0 = ((int)blockIdx.z * (int)(blockDim.x >> 6) + wave) * 16 * a.tiles_per_wave;
    if (k0 >= a.K) return;
    const int nto = min(TO, (a.Dout - o0 + 15) >> 4);
    const int ntk = min(a.tiles_per_wave, (a.K - k0 + 15) >> 4);
    // columns that do not exist read column 0 of the row (valid memory); their accumulators are never stored
    int ocol[TO], kcol[TK];
#pragma unroll
    for (int t = 0; t < TO; ++t) ocol[t] = (o0 + 16 * t + i < a.Dout) ? o0 + 16 * t + i : 0;
#pragma unroll
    for (int t = 0; t < TK; ++t) kcol[t] = (k0 + 16 * t + i < a.K) ? k0 + 16 * t + i : 0;
    f32x4 acc[TO][TK];
#pragma unroll
    for (int t = 0; t < TO; ++t)
#pragma unroll
        for (int u = 0; u < TK; ++u) acc[t][u] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    const bool do_db = a.part_b != nullptr && wave == 0 && blockIdx.z == 0;   // db rides along on the dz operands of one wave
    float dbacc[TO];
#pragma unroll
    for (int t = 0; t < TO; ++t) dbacc[t] = 0.0f;
    int64_t n0, n1;
    grouped_slab(a, blockIdx.x, n0, n1);
    if (n0 < n1) {
        const int64_t nb = (n1 - n0 + 3) >> 2;
        // rows past the slab's end re-read its last row and are replaced by zeros (a select, not a product: 0 * Inf is a NaN)
        auto load = [&](int64_t b, float (&av)[TO], float (&bv)[TK]) {
            const int64_t row = n0 + 4 * b + q;
            const bool in = row < n1;
            const float *pa = a.dz + min(row, n1 - 1) * a.lddz;
            const float *pb = a.x + min(row, n1 - 1) * a.ldx;
#pragma unroll
            for (int t = 0; t < TO; ++t) av[t] = in ? pa[ocol[t]] : 0.0f;
#pragma unroll
            for (int t = 0; t < TK; ++t) bv[t] = in ? pb[kcol[t]] : 0.0f;
        };
        float av[2][TO], bv[2][TK];
        load(0, av[0], bv[0]);
        for (int64_t b = 0; b < nb; b += 2) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                if (b + h < nb) {
                    load(min(b + h + 1, nb - 1), av[h ^ 1], bv[h ^ 1]);
#pragma unroll
                    for (int t = 0; t < TO; ++t) {
                        if (t < nto) {
#pragma unroll
                            for (int u = 0; u < TK; ++u)
                                if (u < ntk) acc[t][u] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[h][t], bv[h][u], acc[t][u], 0, 0, 0);
                        }
                    }
                    if (do_db) {
#pragma unroll
                        for (int t = 0; t < TO; ++t) dbacc[t] = dbacc[t] + av[h][t];
                    }
                }
            }
        }
    }
    if (do_db) {   // rows n + q, q = 0..3, of every batch sit in four lane groups: folded in a fixed order
#pragma unroll
        for (int t = 0; t < TO; ++t) {
            float v = dbacc[t];
            v = v + __shfl_xor(v, 16, 64);
            v = v + __shfl_xor(v, 32, 64);
            if (q == 0 && o0 + 16 * t + i < a.Dout) a.part_b[(int64_t)blockIdx.x * a.Dout + o0 + 16 * t + i] = v;
        }
    }
    // C/D layout: col = lane & 15, row = 4 (lane >> 4) + reg
    float *part = a.part_w + (int64_t)blockIdx.x * a.Dout * a.K;
#pragma unroll
    for (int t = 0; t < TO; ++t) {
        if (t >= nto) continue;
#pragma unroll
        for (int u = 0; u < TK; ++u) {
            if (u >= ntk) continue;
            const int col = k0 + 16 * u + i;
            if (col >= a.K) continue;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = o0 + 16 * t + 4 * q + r;
                if (row < a.Dout) part[(int64_t)row * a.K + col] = acc[t][u][r];
            }
        }
    }
}

// any shape: one thread an element of the slab's partial — dW[o][k], then db[o] — summed over the slab's rows in order
__global__ void __launch_bounds__(256) grouped_gradw_fma_kernel(const GroupedGradArgs a) {
    int64_t n0, n1;
    grouped_slab(a, blockIdx.x, n0, n1);
    const int64_t lenw = a.part_w ? (int64_t)a.Dout * a.K : 0;
    const int64_t total = lenw + (a.part_b ? a.Dout : 0);
    for (int64_t idx = (int64_t)blockIdx.y * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.y * 256) {
        float acc = 0.0f;
        if (idx < lenw) {
            const int64_t o = idx / a.K, k = idx - o * a.K;
            for (int64_t r = n0; r < n1; ++r) acc = fmaf(a.dz[r * a.lddz + o], a.x[r * a.ldx + k], acc);
            a.part_w[(int64_t)blockIdx.x * lenw + idx] = acc;
        } else {
            const int64_t o = idx - lenw;
            for (int64_t r = n0; r < n1; ++r) acc = acc + a.dz[r * a.lddz + o];
            a.part_b[(int64_t)blockIdx.x * a.Dout + o] = acc;
        }
    }
}

struct GroupedFoldArgs {
    const float *part_w, *part_b;
    int64_t G;
    int S;
    int64_t lenw;      // Dout * K, 0 without dW
    int Dout;
    float *dW;
    int64_t dw_stride;
    float *db;         // null: none
    int64_t db_stride; // 0: one column sum over all rows, folded by the extra block row g == G
};
// block row g < G: dW[g] and db[g] = the S partials of group g added in slab order; block row G (a shared db): all G * S partials in order
__global__ void __launch_bounds__(256) grouped_fold_kernel(const GroupedFoldArgs a) {
    const int64_t g = blockIdx.x;
    const int64_t first = (int64_t)blockIdx.y * 256 + threadIdx.x, step = (int64_t)gridDim.y * 256;
    if (g == a.G) {
        for (int64_t o = first; o < a.Dout; o += step) {
            float acc = 0.0f;
            for (int64_t p = 0; p < a.G * a.S; ++p) acc = acc + a.part_b[p * a.Dout + o];
            a.db[o] = acc;
        }
        return;
    }
    const int64_t total = a.lenw + ((a.db && a.db_stride > 0) ? a.Dout : 0);
    for (int64_t idx = first; idx < total; idx += step) {
        float acc = 0.0f;
        if (idx < a.lenw) {
            for (int s = 0; s < a.S; ++s) acc = acc + a.part_w[(g * a.S + s) * a.lenw + idx];
            a.dW[g * a.dw_stride + idx] = acc;
        } else {
            const int64_t o = idx - a.lenw;
            for (int s = 0; s < a.S; ++s) acc = acc + a.part_b[(g * a.S + s) * a.Dout + o];
            a.db[g * a.db_stride + o] = acc;
        }
    }
}

// the calling thread's route record: {kernel, ncb | slabs, waves, grid_x} of its last grouped call
static int (&grouped_route_record())[4] {
    static thread_local int r[4] = {0, 0, 0, 0};
    return r;
}

template <int NCB>
static int launch_grouped_t16(const GroupedArgs &a, const GroupedRoute &r, hipStream_t stream) {
    GNNMP_LDS_OPTIN("grouped_t16_kernel", &grouped_t16_kernel<NCB>);
    grouped_t16_kernel<NCB><<<dim3(r.grid_x, r.grid_y), 64 * r.waves, r.lds_bytes, stream>>>(a);
    GNNMP_LAUNCH_CHECK("grouped_t16_kernel");
    return GNNMP_OK;
}

static bool al16(const void *p, int64_t ld) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0 && (ld & 3) == 0; }

}  // namespace gnnmp

using namespace gnnmp;

extern "C" int gnnmp_debug_grouped_dense_route(int info[4]) {
    if (!info) return fail(GNNMP_EINVAL, "gnnmp_debug_grouped_dense_route: null pointer");
    std::copy(grouped_route_record(), grouped_route_record() + 4, info);
    return GNNMP_OK;
}

extern "C" int gnnmp_grouped_dense_f32(const gnnmp_grouped_dense_t *job, int64_t N, int64_t G, int64_t K, int64_t Dout, gnnmp_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    int(&rec)[4] = grouped_route_record();
    std::fill(rec, rec + 4, 0);
    if (!job) return fail(GNNMP_EINVAL, "grouped_dense: null job");
    if (N < 0 || G < 0 || K <= 0 || Dout <= 0 || K > (1 << 20) || Dout > (1 << 20)) return fail(GNNMP_EINVAL, "grouped_dense: bad size");
    if (job->w_layout != 0 && job->w_layout != 1) return fail(GNNMP_EINVAL, "grouped_dense: bad w_layout %d", job->w_layout);
    if (job->act != GNNMP_ACT_IDENTITY && job->act != GNNMP_ACT_RELU) return fail(GNNMP_EINVAL, "grouped_dense: bad act %d", job->act);
    if (job->ldx < K) return fail(GNNMP_EINVAL, "grouped_dense: ldx = %lld is less than K = %lld", (long long)job->ldx, (long long)K);
    if (job->ldo < Dout) return fail(GNNMP_EINVAL, "grouped_dense: ldo = %lld is less than Dout = %lld", (long long)job->ldo, (long long)Dout);
    if (job->ldw < (job->w_layout == 0 ? K : Dout))
        return fail(GNNMP_EINVAL, "grouped_dense: ldw = %lld is less than a row of W (%lld)", (long long)job->ldw, (long long)(job->w_layout == 0 ? K : Dout));
    if (job->w_stride < 0) return fail(GNNMP_EINVAL, "grouped_dense: negative w_stride");
    if (job->bias_stride != 0 && job->bias_stride < Dout)
        return fail(GNNMP_EINVAL, "grouped_dense: bias_stride = %lld is neither 0 nor at least Dout = %lld", (long long)job->bias_stride, (long long)Dout);
    if (N > 0 && G == 0) return fail(GNNMP_EINVAL, "grouped_dense: %lld rows but no group", (long long)N);
    if (N == 0) return GNNMP_OK;
    if (!job->x || !job->W || !job->seg_ptr || !job->out) return fail(GNNMP_EINVAL, "grouped_dense: null pointer");
    const WStrides ws = w_strides(job->w_layout, job->ldw);
    GroupedArgs a;
    a.x = job->x; a.ldx = job->ldx;
    a.W = job->W; a.w_stride = job->w_stride; a.sj = ws.sj; a.sk = ws.sk;
    a.bias = job->bias; a.bias_stride = job->bias_stride;
    a.seg_ptr = job->seg_ptr; a.G = G;
    a.act = job->act;
    a.out = job->out; a.ldo = job->ldo;
    a.N = N; a.K = (int)K; a.Dout = (int)Dout;
    const GroupedShape shape{N, G, K, Dout, al16(job->x, job->ldx), al16(job->out, job->ldo)};
    const GroupedRoute r = grouped_plan(shape, device_cus());
    a.waves = r.waves;
    a.per_block = r.tiles_per_block;
    int rc;
    if (r.kernel == GROUPED_T16) {
        switch (r.ncb) {
            case 8: rc = launch_grouped_t16<8>(a, r, stream); break;
            case 7: rc = launch_grouped_t16<7>(a, r, stream); break;
            case 6: rc = launch_grouped_t16<6>(a, r, stream); break;
            case 4: rc = launch_grouped_t16<4>(a, r, stream); break;
            case 2: rc = launch_grouped_t16<2>(a, r, stream); break;
            default: rc = fail(GNNMP_EUNSUPPORTED, "grouped_dense: no instance <%d>", r.ncb); break;
        }
    } else {
        grouped_fma_kernel<<<r.grid_x, 256, 0, stream>>>(a);
        GNNMP_LAUNCH_CHECK("grouped_fma_kernel");
        rc = GNNMP_OK;
    }
    if (rc == GNNMP_OK) {   // the record says what was launched
        const int v[4] = {r.kernel, r.ncb, r.waves, (int)r.grid_x};
        std::copy(v, v + 4, rec);
    }
    return rc;
}

extern "C" int64_t gnnmp_grouped_dense_grad_workspace(int64_t N, int64_t G, int64_t Dout, int64_t K) {
    if (N < 0 || G <= 0 || Dout <= 0 || K <= 0) return 0;
    return grouped_grad_workspace(N, G, Dout, K, device_cus());
}

extern "C" int gnnmp_grouped_dense_grad_w_f32(const gnnmp_grouped_dense_grad_t *job, int64_t N, int64_t G, int64_t K, int64_t Dout,
                                              gnnmp_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    int(&rec)[4] = grouped_route_record();
    std::fill(rec, rec + 4, 0);
    if (!job) return fail(GNNMP_EINVAL, "grouped_dense_grad_w: null job");
    if (N < 0 || G < 0 || K <= 0 || Dout <= 0 || K > (1 << 16) || Dout > (1 << 16) || G > (int64_t)INT32_MAX / 1024)
        return fail(GNNMP_EINVAL, "grouped_dense_grad_w: bad size");
    if (!job->dW && !job->db) return fail(GNNMP_EINVAL, "grouped_dense_grad_w: nothing to compute");
    if (job->lddz < Dout) return fail(GNNMP_EINVAL, "grouped_dense_grad_w: lddz = %lld is less than Dout = %lld", (long long)job->lddz, (long long)Dout);
    if (job->dW && job->ldx < K) return fail(GNNMP_EINVAL, "grouped_dense_grad_w: ldx = %lld is less than K = %lld", (long long)job->ldx, (long long)K);
    if (job->dW && job->dw_stride < Dout * K)
        return fail(GNNMP_EINVAL, "grouped_dense_grad_w: dw_stride = %lld is less than Dout * K = %lld", (long long)job->dw_stride, (long long)(Dout * K));
    if (job->db && job->db_stride != 0 && job->db_stride < Dout)
        return fail(GNNMP_EINVAL, "grouped_dense_grad_w: db_stride = %lld is neither 0 nor at least Dout = %lld", (long long)job->db_stride, (long long)Dout);
    if (N > 0 && G == 0) return fail(GNNMP_EINVAL, "grouped_dense_grad_w: %lld rows but no group", (long long)N);
    if (G == 0) return GNNMP_OK;
    if (!job->seg_ptr || !job->workspace || (N > 0 && (!job->dz || (job->dW && !job->x)))) return fail(GNNMP_EINVAL, "grouped_dense_grad_w: null pointer");
    const int cus = device_cus();
    const int64_t need = grouped_grad_workspace(N, G, Dout, K, cus);
    if (job->workspace_floats < need)
        return fail(GNNMP_EINVAL, "grouped_dense_grad_w: workspace too small (%lld < %lld floats)", (long long)job->workspace_floats, (long long)need);
    const GroupedShape shape{N, G, K, Dout, al16(job->dz, job->lddz) && al16(job->x, job->ldx), true};
    const GroupedGradRoute r = grouped_grad_plan(shape, job->dW != nullptr, cus);
    GroupedGradArgs a;
    a.dz = job->dz; a.lddz = job->lddz;
    a.x = job->x; a.ldx = job->ldx;
    a.seg_ptr = job->seg_ptr;
    a.N = N; a.G = G; a.S = r.slabs;
    a.part_w = job->dW ? job->workspace : nullptr;
    a.part_b = job->db ? job->workspace + G * r.slabs * Dout * K : nullptr;
    a.Dout = (int)Dout; a.K = (int)K;
    a.tiles_per_wave = r.tiles_per_wave;
    if (r.kernel == GROUPED_GRADW16) {
        const dim3 grid(r.grid_x, r.grid_y, r.grid_z);
        if ((Dout + 15) / 16 <= 4)
            grouped_gradw16_kernel<4, 4><<<grid, 64 * r.waves, 0, stream>>>(a);
        else
            grouped_gradw16_kernel<8, 4><<<grid, 64 * r.waves, 0, stream>>>(a);
        GNNMP_LAUNCH_CHECK("grouped_gradw16_kernel");
    } else {
        grouped_gradw_fma_kernel<<<dim3(r.grid_x, r.grid_y), 256, 0, stream>>>(a);
        GNNMP_LAUNCH_CHECK("grouped_gradw_fma_kernel");
    }
    GroupedFoldArgs f;
    f.part_w = a.part_w; f.part_b = a.part_b;
    f.G = G; f.S = r.slabs;
    f.lenw = job->dW ? Dout * K : 0;
    f.Dout = (int)Dout;
    f.dW = job->dW; f.dw_stride = job->dw_stride;
    f.db = job->db; f.db_stride = job->db_stride;
    const bool shared_db = job->db && job->db_stride == 0;
    grouped_fold_kernel<<<dim3((unsigned)(G + (shared_db ? 1 : 0)), r.fold_y), 256, 0, stream>>>(f);
    GNNMP_LAUNCH_CHECK("grouped_fold_kernel");
    const int v[4] = {r.kernel, r.slabs, r.waves, (int)r.grid_x};
    std::copy(v, v + 4, rec);
    return GNNMP_OK;
}
