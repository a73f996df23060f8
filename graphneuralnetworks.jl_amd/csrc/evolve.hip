// evolve.hip — Flux.LSTMCell at BATCH ONE on a vector as long as a flattened convolution weight: the recurrence of EvolveGCNOCell
// (GraphNeuralNetworks/src/layers/temporalconv.jl:678-705), forward and pullback.  D = in * out, Wi and Wh are [4D][D]: a step is two
// matrix-vector products that read 8 D^2 floats for 2 D^2 multiply-adds each way — bandwidth, nothing else — and the dense family
// (MFMA tiles over many rows, the weight staged in LDS) has no route for one row.  include/gnnmp.h states the arithmetic.
//   lstm_matvec_cell_kernel   one lane group (<= a wave) owns element j: it streams the eight rows j, D + j, 2D + j, 3D + j of Wi and Wh
//                             against x and h — VEC floats a lane and row, all eight rows of a pass in flight before the first is used —
//                             folds the four pre-activations across the group with an xor butterfly and finishes the gates itself: the
//                             [4D] intermediate is never read back.  A wave streams 8 KB a pass at VEC = 4; D waves are in flight.
//                             D <= 2048: D waves do not fill the chip, and a row that fills 256 lanes goes to a whole workgroup (WIDE:
//                             one element a block, the four waves' sums added in wave order through LDS) — 11 against 14.7 us at D = 1024
//   lstm_matvec_grad_kernel   Wi' da and Wh' da: a thread owns VEC columns and walks a slab of rows — a wave reads 64 VEC consecutive
//                             floats of one row, ROWS_IN_FLIGHT rows at once — and writes its partial to part[matrix][slab][k]
//   lstm_matvec_fold_kernel   the second launch: out[k] = Σ_slab part, slabs ascending (x first, then h when the two are summed), + addend
//   outer_accum_kernel        dW[r][k] = Σ_t A[t][r] B[t][k], t ascending: a thread owns VEC columns of OUTER_ROWS rows, B[t] is loaded
//                             once for all of them, every row is stored as whole 16-byte lanes side by side; write-bound
// Rows are D floats long: a row is 16-byte aligned only when D % 4 == 0, so VEC comes from pick_vec / narrow_vec over D and every pointer
// a kernel touches with vector accesses.  No atomics; no workgroup waits on another (the fold across slabs is a launch of its own); every
// output element written once; element offsets are 64-bit (4D * D passes 2^31 at D = 23 171).  -ffp-contract=off: nothing is fused.
#include "common.h"

namespace gnnmp {

namespace {

constexpr int64_t EVOLVE_MAX_D = (int64_t)1 << 20;
constexpr int64_t CELL_WIDE_MAX_D = 2048;
constexpr int GRAD_MAX_SLABS = 256;     // slabs the 4D rows of a matrix are cut into (gnnmp_lstm_matvec_grad_workspace: 2 * slabs * D)
constexpr int GRAD_MIN_SLAB_ROWS = 16;
constexpr int ROWS_IN_FLIGHT = 4;
constexpr int OUTER_ROWS = 8;

__device__ __forceinline__ float ev_sigmoid(float x) {     // NNlib.σ, lstm_pointwise_kernel's expression (leaf.hip)
    const float t = expf(-fabsf(x));
    return x >= 0.0f ? 1.0f / (1.0f + t) : t / (1.0f + t);
}

struct MatvecCellArgs {
    const float *Wi, *Wh, *x, *h, *c, *b;
    float *h_out, *c_out, *a_out;
    int64_t D;
    int log2g;
};

// WIDE: the lane group is the whole 256-thread workgroup (one element a block) — for a D too small to fill the chip with one wave an
// element; the four waves' sums meet in LDS and are added in wave order
template <int VEC, bool WIDE>
__global__ void __launch_bounds__(256) lstm_matvec_cell_kernel(const MatvecCellArgs k) {
    const int G = WIDE ? 256 : 1 << k.log2g;
    const int lig = threadIdx.x & (G - 1);
    const int64_t D = k.D;
    const int64_t j = WIDE ? (int64_t)blockIdx.x : ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> k.log2g;
    const bool live = j < D;                      // a dead group (the last block's tail) walks row 0 and stores nothing: every lane of a
    const int64_t jj = live ? j : 0;              // wave stays in the butterflies
    const bool has_h = k.h != nullptr;
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int64_t f = (int64_t)lig * VEC; f < D; f += (int64_t)G * VEC) {
        float wi[4][VEC], wh[4][VEC], xv[VEC], hv[VEC];
#pragma unroll
        for (int q = 0; q < 4; ++q) Vec<VEC>::load(k.Wi + ((int64_t)q * D + jj) * D + f, wi[q]);
        if (has_h) {
#pragma unroll
            for (int q = 0; q < 4; ++q) Vec<VEC>::load(k.Wh + ((int64_t)q * D + jj) * D + f, wh[q]);
            Vec<VEC>::load(k.h + f, hv);
        }
        Vec<VEC>::load(k.x + f, xv);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
#pragma unroll
            for (int v = 0; v < VEC; ++v) acc[q] = acc[q] + wi[q][v] * xv[v];
        }
        if (has_h) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
#pragma unroll
                for (int v = 0; v < VEC; ++v) acc[q] = acc[q] + wh[q][v] * hv[v];
            }
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        for (int o = (G < 64 ? G : 64) >> 1; o > 0; o >>= 1) acc[q] = acc[q] + __shfl_xor(acc[q], o, 64);
    }
    if (WIDE) {                                   // every thread of the block is here: the grid is exactly D blocks
        __shared__ float red[4][4];
        if ((threadIdx.x & 63) == 0) {
#pragma unroll
            for (int q = 0; q < 4; ++q) red[threadIdx.x >> 6][q] = acc[q];
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] = ((red[0][q] + red[1][q]) + red[2][q]) + red[3][q];
    }
    if (!live || lig != 0) return;
    float a[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) a[q] = acc[q] + (k.b ? k.b[(int64_t)q * D + j] : 0.0f);
    const float cv = k.c ? k.c[j] : 0.0f;
    const float cn = ev_sigmoid(a[1]) * cv + ev_sigmoid(a[0]) * tanhf(a[2]);
    k.c_out[j] = cn;
    k.h_out[j] = ev_sigmoid(a[3]) * tanhf(cn);
    if (k.a_out) {
#pragma unroll
        for (int q = 0; q < 4; ++q) k.a_out[(int64_t)q * D + j] = a[q];
    }
}

struct MatvecGradArgs {
    const float *W[2];       // Wi, Wh; a matrix that is not wanted is null and its grid.z slice does not exist
    const float *da;
    float *part;             // [2][slabs][D]
    int64_t D;
    int slabs, slab_rows, first;      // grid.z index z is matrix first + z
};

template <int VEC>
__global__ void __launch_bounds__(256) lstm_matvec_grad_kernel(const MatvecGradArgs k) {
    const int64_t D = k.D, R = 4 * D;
    const int m = k.first + (int)blockIdx.z;
    const int64_t f = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * VEC;
    if (f >= D) return;
    const float *W = k.W[m];
    const int64_t r0 = (int64_t)blockIdx.y * k.slab_rows;
    const int64_t r1 = r0 + k.slab_rows < R ? r0 + k.slab_rows : R;
    float acc[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) acc[v] = 0.0f;
    for (int64_t r = r0; r < r1; r += ROWS_IN_FLIGHT) {
        float w[ROWS_IN_FLIGHT][VEC], d[ROWS_IN_FLIGHT];
#pragma unroll
        for (int u = 0; u < ROWS_IN_FLIGHT; ++u) {
            const int64_t rr = r + u < r1 ? r + u : r1 - 1;      // clamped: loaded, not added
            Vec<VEC>::load(W + rr * D + f, w[u]);
            d[u] = k.da[rr];
        }
#pragma unroll
        for (int u = 0; u < ROWS_IN_FLIGHT; ++u) {
            if (r + u < r1) {
#pragma unroll
                for (int v = 0; v < VEC; ++v) acc[v] = acc[v] + w[u][v] * d[u];
            }
        }
    }
    Vec<VEC>::store(k.part + ((int64_t)m * k.slabs + blockIdx.y) * D + f, acc);      // an empty slab (r0 >= R) stores zeros
}

struct MatvecFoldArgs {
    const float *part, *add_x, *add_h;
    float *out_x, *out_h;
    int64_t D;
    int slabs, sum;
};

__global__ void __launch_bounds__(256) lstm_matvec_fold_kernel(const MatvecFoldArgs k) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= k.D) return;
    float s[2] = {0.0f, 0.0f};
    for (int m = 0; m < 2; ++m) {
        if (!(k.sum || (m == 0 ? k.out_x : k.out_h))) continue;
        const float *p = k.part + (int64_t)m * k.slabs * k.D + i;
        for (int b = 0; b < k.slabs; ++b) s[m] = s[m] + p[(int64_t)b * k.D];
    }
    if (k.sum) {
        float v = s[0] + s[1];
        if (k.add_x) v = v + k.add_x[i];
        k.out_x[i] = v;
        return;
    }
    if (k.out_x) k.out_x[i] = k.add_x ? s[0] + k.add_x[i] : s[0];
    if (k.out_h) k.out_h[i] = k.add_h ? s[1] + k.add_h[i] : s[1];
}

struct OuterArgs {
    const float *A, *B;
    float *dW, *db;
    int64_t T, R, K;
};

template <int VEC>
__global__ void __launch_bounds__(256) outer_accum_kernel(const OuterArgs k) {
    const int64_t r0 = (int64_t)blockIdx.x * OUTER_ROWS;
    const int64_t f = ((int64_t)blockIdx.y * blockDim.x + threadIdx.x) * VEC;
    const int nr = (int)(k.R - r0 < OUTER_ROWS ? k.R - r0 : OUTER_ROWS);
    if (k.db && blockIdx.y == 0 && (int)threadIdx.x < nr) {
        float s = 0.0f;
        for (int64_t t = 0; t < k.T; ++t) s = s + k.A[t * k.R + r0 + threadIdx.x];
        k.db[r0 + threadIdx.x] = s;
    }
    if (f >= k.K) return;
    float acc[OUTER_ROWS][VEC];
#pragma unroll
    for (int u = 0; u < OUTER_ROWS; ++u) {
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[u][v] = 0.0f;
    }
    for (int64_t t = 0; t < k.T; ++t) {
        float bv[VEC];
        Vec<VEC>::load(k.B + t * k.K + f, bv);
#pragma unroll
        for (int u = 0; u < OUTER_ROWS; ++u) {
            const float a = k.A[t * k.R + r0 + (u < nr ? u : 0)];      // uniform over the block
#pragma unroll
            for (int v = 0; v < VEC; ++v) acc[u][v] = acc[u][v] + a * bv[v];
        }
    }
#pragma unroll
    for (int u = 0; u < OUTER_ROWS; ++u) {
        if (u < nr) Vec<VEC>::store(k.dW + (r0 + u) * k.K + f, acc[u]);
    }
}

// [p, p + n floats) meets [q, q + m floats); a null pointer meets nothing
bool spans_meet(const float *p, int64_t n, const float *q, int64_t m) {
    if (!p || !q || n <= 0 || m <= 0) return false;
    const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
    return a < b + (uintptr_t)m * 4 && b < a + (uintptr_t)n * 4;
}

int grad_slabs(int64_t D) {
    const int64_t s = 4 * D / GRAD_MIN_SLAB_ROWS;
    return (int)(s < 1 ? 1 : s > GRAD_MAX_SLABS ? GRAD_MAX_SLABS : s);
}

int check_D(const char *who, int64_t D) {
    if (D < 0 || D > EVOLVE_MAX_D) return fail(GNNMP_EINVAL, "%s: bad D %lld (0 .. 2^20)", who, (long long)D);
    return GNNMP_OK;
}

}  // namespace
}  // namespace gnnmp

using namespace gnnmp;

extern "C" {

int gnnmp_lstm_matvec_cell_f32(const gnnmp_lstm_matvec_t *job, int64_t D, gnnmp_stream_t stream) {
    const char *who = "lstm_matvec_cell";
    if (!job) return fail(GNNMP_EINVAL, "%s: null job", who);
    GNNMP_TRY(check_D(who, D));
    if (D == 0) return GNNMP_OK;
    if (!job->Wi || !job->x) return fail(GNNMP_EINVAL, "%s: null Wi or x", who);
    if (job->h && !job->Wh) return fail(GNNMP_EINVAL, "%s: h without Wh", who);
    if (!job->h_out || !job->c_out) return fail(GNNMP_EINVAL, "%s: null h_out or c_out", who);
    const struct { const char *name; const float *p; int64_t n; } outs[] = {{"h_out", job->h_out, D}, {"c_out", job->c_out, D},
                                                                            {"a_out", job->a_out, 4 * D}};
    const struct { const char *name; const float *p; } ins[] = {{"x", job->x}, {"h", job->h}, {"c", job->c}};
    for (const auto &o : outs) {
        for (const auto &i : ins) {
            if (spans_meet(o.p, o.n, i.p, D))
                return fail(GNNMP_EINVAL, "%s: %s overlaps %s, which other workgroups still read", who, o.name, i.name);
        }
    }
    if (spans_meet(job->h_out, D, job->c_out, D) || spans_meet(job->a_out, 4 * D, job->h_out, D) ||
        spans_meet(job->a_out, 4 * D, job->c_out, D))
        return fail(GNNMP_EINVAL, "%s: h_out, c_out and a_out overlap each other", who);
    // the wide-load path by alignment: rows start at multiples of D floats from Wi / Wh
    int vec = pick_vec(D, job->Wi, job->x);
    vec = narrow_vec(vec, job->h ? job->Wh : nullptr, job->h);
    MatvecCellArgs k = {job->Wi, job->Wh, job->x, job->h, job->c, job->b, job->h_out, job->c_out, job->a_out, D, 0};
    k.log2g = pick_log2g((D + vec - 1) / vec);
    // one wave an element is D waves: below CELL_WIDE_MAX_D that is too few to fill the chip, and a row that fills 256 lanes goes to a
    // whole workgroup instead (not while KNOB_FORCE_LOG2G pins the group)
    const bool wide = (D + vec - 1) / vec >= 256 && D <= CELL_WIDE_MAX_D && knob(KNOB_FORCE_LOG2G) < 0;
    const int64_t nb = wide ? D : ((D << k.log2g) + 255) / 256;
    if (nb >= INT32_MAX) return fail(GNNMP_EUNSUPPORTED, "%s: D too large (%lld)", who, (long long)D);
    with_vec(vec, [&](auto V) {
        if (wide)
            lstm_matvec_cell_kernel<decltype(V)::value, true><<<(unsigned)nb, 256, 0, (hipStream_t)stream>>>(k);
        else
            lstm_matvec_cell_kernel<decltype(V)::value, false><<<(unsigned)nb, 256, 0, (hipStream_t)stream>>>(k);
    });
    GNNMP_LAUNCH_CHECK("lstm_matvec_cell_kernel");
    return GNNMP_OK;
}

int64_t gnnmp_lstm_matvec_grad_workspace(int64_t D) {
    if (D <= 0 || D > EVOLVE_MAX_D) return 0;
    return 2 * (int64_t)grad_slabs(D) * D;
}

int gnnmp_lstm_matvec_grad_f32(const gnnmp_lstm_matvec_grad_t *job, int64_t D, gnnmp_stream_t stream) {
    const char *who = "lstm_matvec_grad";
    if (!job) return fail(GNNMP_EINVAL, "%s: null job", who);
    GNNMP_TRY(check_D(who, D));
    if (job->sum != 0 && job->sum != 1) return fail(GNNMP_EINVAL, "%s: bad sum %d (0 or 1)", who, job->sum);
    if (D == 0) return GNNMP_OK;
    if (!job->da) return fail(GNNMP_EINVAL, "%s: null da", who);
    if (!job->out_x && !job->out_h) return fail(GNNMP_EINVAL, "%s: out_x and out_h are both null", who);
    if (job->sum && (!job->out_x || job->out_h || job->add_h))
        return fail(GNNMP_EINVAL, "%s: sum = 1 writes out_x alone (out_h and add_h must be null)", who);
    const bool need_i = job->sum || job->out_x, need_h = job->sum || job->out_h;
    if ((need_i && !job->Wi) || (need_h && !job->Wh)) return fail(GNNMP_EINVAL, "%s: null Wi or Wh", who);
    if ((job->add_x && !job->out_x) || (job->add_h && !job->out_h)) return fail(GNNMP_EINVAL, "%s: an addend without its output", who);
    const int64_t need = gnnmp_lstm_matvec_grad_workspace(D);
    if (!job->ws || job->ws_floats < need)
        return fail(GNNMP_EINVAL, "%s: workspace of %lld floats, %lld needed", who, (long long)(job->ws ? job->ws_floats : 0), (long long)need);
    const struct { const char *name; const float *p; } outs[] = {{"out_x", job->out_x}, {"out_h", job->out_h}};
    for (const auto &o : outs) {
        if (spans_meet(o.p, D, job->da, 4 * D) || spans_meet(o.p, D, job->ws, need))
            return fail(GNNMP_EINVAL, "%s: %s overlaps da or the workspace", who, o.name);
    }
    if (spans_meet(job->out_x, D, job->out_h, D)) return fail(GNNMP_EINVAL, "%s: out_x overlaps out_h", who);
    if (spans_meet(job->ws, need, job->da, 4 * D) || spans_meet(job->ws, need, job->add_x, D) || spans_meet(job->ws, need, job->add_h, D))
        return fail(GNNMP_EINVAL, "%s: the workspace overlaps da or an addend", who);
    MatvecGradArgs k = {{job->Wi, job->Wh}, job->da, job->ws, D, grad_slabs(D), 0, need_i ? 0 : 1};
    k.slab_rows = (int)((4 * D + k.slabs - 1) / k.slabs);
    int vec = pick_vec(D, need_i ? job->Wi : nullptr, need_h ? job->Wh : nullptr);
    vec = narrow_vec(vec, job->ws);
    const int64_t ct = ((D + vec - 1) / vec + 255) / 256;
    const dim3 grid((unsigned)ct, (unsigned)k.slabs, (unsigned)((need_i ? 1 : 0) + (need_h ? 1 : 0)));
    with_vec(vec, [&](auto V) { lstm_matvec_grad_kernel<decltype(V)::value><<<grid, 256, 0, (hipStream_t)stream>>>(k); });
    GNNMP_LAUNCH_CHECK("lstm_matvec_grad_kernel");
    const MatvecFoldArgs f = {job->ws, job->add_x, job->add_h, job->out_x, job->out_h, D, k.slabs, job->sum};
    lstm_matvec_fold_kernel<<<(unsigned)((D + 255) / 256), 256, 0, (hipStream_t)stream>>>(f);
    GNNMP_LAUNCH_CHECK("lstm_matvec_fold_kernel");
    return GNNMP_OK;
}

int gnnmp_outer_accum_f32(const gnnmp_outer_accum_t *job, int64_t T, int64_t R, int64_t K, gnnmp_stream_t stream) {
    const char *who = "outer_accum";
    if (!job) return fail(GNNMP_EINVAL, "%s: null job", who);
    if (T < 0 || T > ((int64_t)1 << 20)) return fail(GNNMP_EINVAL, "%s: bad T %lld (0 .. 2^20)", who, (long long)T);
    if (R < 0 || R > 4 * EVOLVE_MAX_D) return fail(GNNMP_EINVAL, "%s: bad R %lld (0 .. 2^22)", who, (long long)R);
    if (K < 0 || K > EVOLVE_MAX_D) return fail(GNNMP_EINVAL, "%s: bad K %lld (0 .. 2^20)", who, (long long)K);
    if (T == 0 || R == 0 || (K == 0 && !job->db)) return GNNMP_OK;
    if (!job->A) return fail(GNNMP_EINVAL, "%s: null A", who);
    if (K > 0 && (!job->B || !job->dW)) return fail(GNNMP_EINVAL, "%s: null B or dW", who);
    if (spans_meet(job->dW, R * K, job->A, T * R) || spans_meet(job->dW, R * K, job->B, T * K) || spans_meet(job->dW, R * K, job->db, R) ||
        spans_meet(job->db, R, job->A, T * R) || spans_meet(job->db, R, job->B, T * K))
        return fail(GNNMP_EINVAL, "%s: an output overlaps an input or the other output", who);
    const int vec = K > 0 ? pick_vec(K, job->B, job->dW) : 1;
    const int64_t ct = K > 0 ? ((K + vec - 1) / vec + 255) / 256 : 1;
    const dim3 grid((unsigned)((R + OUTER_ROWS - 1) / OUTER_ROWS), (unsigned)ct);
    const OuterArgs k = {job->A, job->B, job->dW, job->db, T, R, K};
    with_vec(vec, [&](auto V) { outer_accum_kernel<decltype(V)::value><<<grid, 256, 0, (hipStream_t)stream>>>(k); });
    GNNMP_LAUNCH_CHECK("outer_accum_kernel");
    return GNNMP_OK;
}

}  // extern "C"
