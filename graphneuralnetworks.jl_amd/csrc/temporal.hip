// temporal.hip — TGCN's recurrence (GraphNeuralNetworks/src/layers/temporalconv.jl:809-849, scanned over time by GNNRecurrence,
// :121-135) after the graph convolutions of all T steps have been done up front (they depend on x_t only, never on the state).
// What is left per step is node-local:
//   a_zr = P_zr[t] + U_zr h,  z = σ(a_z), r = σ(a_r),  h~ = tanh(P_h[t] + U_h (r .* h)),  h' = (1 - z) .* h + z .* h~
// with P[n][t] = W_g[:, 1:out] * conv_g(x_t) + b_g (the input half of dense_g, computed by the caller) and U_g = W_g[:, out+1:2out].
//
// gnnmp_tgcn_recurrence_f32 runs all T steps for 16 nodes per wave in ONE launch.  The products are formed transposed on
// v_mfma_f32_16x16x4_f32 exactly as in mfma16.h (A = a 16-row block of U, B = 16 nodes of the state): in the C/D layout lane (n, q)
// holds gate columns 16 m + 4 q .. + 3 of node n, and with k-slot q of step (j, i) defined as k = 16 j + 4 q + i the B operand of the
// next product is that same register — the state never leaves the registers and never needs a re-layout between steps.
//
// U lives in LDS as fragments of 1 KB: fragment f = (g, m, j) holds, for lane l and i = 0..3, U_g[16 m + (l & 15)][16 j + 4 (l >> 4) + i]
// (the pullback's transposed image: U_g[16 j + 4 (l >> 4) + i][16 m + (l & 15)]), so one ds_read_b128 per lane feeds four steps.
// 3 NT^2 fragments for NT = ceil(out / 16) tiles: out = 100 (NT = 7) is 147 KB, inside the 160 KiB of a CU; out in 113..128 (NT = 8,
// 192 KB) keeps the first 160 fragments in LDS and reads the last 32 (the lower half of U_h) from L2 on every step.  One block per CU.
#include "common.h"
#include "mfma16.h"

namespace gnnmp {

namespace {

constexpr int TGCN_MAX_OUT = 128;
constexpr int TGCN_LDS_FRAGS = 160;     // 160 KiB of LDS in 1 KB fragments

__device__ __forceinline__ float tg_sigmoid(float x) {     // NNlib.σ: t = exp(-|x|); x >= 0 ? 1 / (1 + t) : t / (1 + t)
    const float t = expf(-fabsf(x));
    return x >= 0.0f ? 1.0f / (1.0f + t) : t / (1.0f + t);
}

// fragment f of the U image, read from the weights as stored (U_zr [2 out][out], U_h [out][out], row-major); zero outside out x out
template <bool BWD>
__device__ __forceinline__ f32x4 tg_frag_global(const float *__restrict__ Uzr, const float *__restrict__ Uh, int out, int NT, int f,
                                                int lane) {
    const int g = f / (NT * NT), rem = f - g * NT * NT, m = rem / NT, j = rem - m * NT;
    const float *U = g < 2 ? Uzr + (int64_t)g * out * out : Uh;
    const int a = 16 * m + (lane & 15), b0 = 16 * j + 4 * (lane >> 4);
    f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int b = b0 + i;
        if (a < out && b < out) v[i] = BWD ? U[(int64_t)b * out + a] : U[(int64_t)a * out + b];
    }
    return v;
}

template <bool BWD>
__device__ __forceinline__ void tg_fill(f32x4 *img, const float *Uzr, const float *Uh, int out, int NT, int nlds) {
    // independent loads, four in flight per thread: a block of 256 threads fills 147 KB in a few L2 round trips
    const int n = nlds * 64;
    for (int idx0 = threadIdx.x; idx0 < n; idx0 += 4 * blockDim.x) {
        f32x4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int idx = idx0 + u * blockDim.x;
            if (idx < n) v[u] = tg_frag_global<BWD>(Uzr, Uh, out, NT, idx >> 6, idx & 63);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int idx = idx0 + u * blockDim.x;
            if (idx < n) img[idx] = v[u];
        }
    }
}

template <int NT>
constexpr int tg_nlds() { return 3 * NT * NT < TGCN_LDS_FRAGS ? 3 * NT * NT : TGCN_LDS_FRAGS; }

// (f is a compile-time constant after unrolling: the LDS / L2 choice costs nothing, and only NT = 8 has L2 fragments at all)
template <int NT, bool BWD>
__device__ __forceinline__ f32x4 tg_frag(const f32x4 *img, const float *Uzr, const float *Uh, int out, int f, int lane) {
    if (f < tg_nlds<NT>()) return img[f * 64 + lane];
    return tg_frag_global<BWD>(Uzr, Uh, out, NT, f, lane);
}

// acc[m] += Σ_j frag(fbase + m NT + j) · b[j] for m < NM: four row blocks at a time, steps i-major (no two consecutive MFMAs on one
// accumulator; mfma16.h: t16_block)
template <int NT, int NM, bool BWD>
__device__ __forceinline__ void tg_prod(f32x4 (&acc)[NM], const f32x4 (&b)[NT], const f32x4 *img, const float *Uzr, const float *Uh,
                                        int out, int fbase, int lane) {
    constexpr int CG = 4;
#pragma unroll
    for (int j = 0; j < NT; ++j) {
#pragma unroll
        for (int m0 = 0; m0 < NM; m0 += CG) {
            f32x4 w[CG];
#pragma unroll
            for (int c = 0; c < CG; ++c)
                if (m0 + c < NM) w[c] = tg_frag<NT, BWD>(img, Uzr, Uh, out, fbase + (m0 + c) * NT + j, lane);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int c = 0; c < CG; ++c)
                    if (m0 + c < NM) acc[m0 + c] = mfma16(w[c][i], b[j][i], acc[m0 + c]);
            // fence for the scheduler: without it every fragment read of the unrolled loops is hoisted to the top and the operands of
            // all of them (3 NT^2 x 4 registers) are live at once — 400+ registers and scratch from NT = 5 on
            __builtin_amdgcn_sched_barrier(0);
        }
    }
}

// four consecutive columns c0 .. c0 + 3 of one row, zero / dropped past `lim`
__device__ __forceinline__ f32x4 tg_load4(const float *p, int c0, int lim) {
    f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (c0 + i < lim) v[i] = p[c0 + i];
    return v;
}
__device__ __forceinline__ void tg_store4(float *p, int c0, int lim, f32x4 v) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (c0 + i < lim) p[c0 + i] = v[i];
}

// state of node n (lane layout: tile j, component i = column 16 j + 4 q + i): h0 NULL = zeros, stride 0 = one vector for every node
template <int NT>
__device__ __forceinline__ void tg_load_h0(f32x4 (&h)[NT], const float *h0, int64_t h0_stride, int64_t node, bool valid, int q, int out) {
#pragma unroll
    for (int j = 0; j < NT; ++j) h[j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    if (h0 && valid) {
#pragma unroll
        for (int j = 0; j < NT; ++j) h[j] = tg_load4(h0 + node * h0_stride, 16 * j + 4 * q, out);
    }
}

template <int NT>
__global__ void __launch_bounds__(256) tgcn_fwd_kernel(const float *__restrict__ P, const float *__restrict__ Uzr,
                                                       const float *__restrict__ Uh, const float *__restrict__ h0, int64_t h0_stride,
                                                       float *__restrict__ y, float *__restrict__ gates, int64_t N, int T, int out) {
    extern __shared__ f32x4 img[];
    tg_fill<false>(img, Uzr, Uh, out, NT, tg_nlds<NT>());
    __syncthreads();
    const int lane = threadIdx.x & 63, n = lane & 15, q = lane >> 4;
    const int64_t node = ((int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * 16 + n;
    const bool valid = node < N;
    if (((int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * 16 >= N) return;    // (wave-uniform)
    f32x4 h[NT];
    tg_load_h0<NT>(h, h0, h0_stride, node, valid, q, out);
    const int64_t D3 = 3 * (int64_t)out;
    for (int t = 0; t < T; ++t) {
        const float *Pt = P + (node * T + t) * D3;
        float *gt = gates ? gates + (node * T + t) * D3 : nullptr;
        f32x4 azr[2 * NT];
#pragma unroll
        for (int m = 0; m < NT; ++m) {
            azr[m] = valid ? tg_load4(Pt, 16 * m + 4 * q, out) : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            azr[NT + m] = valid ? tg_load4(Pt + out, 16 * m + 4 * q, out) : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        }
        tg_prod<NT, 2 * NT, false>(azr, h, img, Uzr, Uh, out, 0, lane);
        // z in place of a_z, r .* h in place of a_r (r goes to the saved gates first)
#pragma unroll
        for (int m = 0; m < NT; ++m) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                azr[m][i] = tg_sigmoid(azr[m][i]);
                azr[NT + m][i] = tg_sigmoid(azr[NT + m][i]);
            }
            if (valid && gt) {
                tg_store4(gt, 16 * m + 4 * q, out, azr[m]);
                tg_store4(gt + out, 16 * m + 4 * q, out, azr[NT + m]);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) azr[NT + m][i] = azr[NT + m][i] * h[m][i];
        }
        f32x4 ah[NT], rh[NT];
#pragma unroll
        for (int m = 0; m < NT; ++m) {
            rh[m] = azr[NT + m];
            ah[m] = valid ? tg_load4(Pt + 2 * out, 16 * m + 4 * q, out) : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        }
        tg_prod<NT, NT, false>(ah, rh, img, Uzr, Uh, out, 2 * NT * NT, lane);
#pragma unroll
        for (int m = 0; m < NT; ++m) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float ht = tanhf(ah[m][i]);
                ah[m][i] = ht;
                h[m][i] = (1.0f - azr[m][i]) * h[m][i] + azr[m][i] * ht;
            }
            if (valid) {
                tg_store4(y + (node * T + t) * out, 16 * m + 4 * q, out, h[m]);
                if (gt) tg_store4(gt + 2 * out, 16 * m + 4 * q, out, ah[m]);
            }
        }
    }
}

// reverse-time pullback of the same recurrence (saved z, r, h~ from the forward, h_{t-1} = y[t-1] or h0):
//   Δh = dy[t] + Δh_carry;  Δa_h = Δh z (1 - h~^2);  Δ(r h) = U_h' Δa_h;  Δa_z = Δh (h~ - h_{t-1}) z (1 - z);  Δa_r = Δ(r h) h_{t-1} r (1 - r)
//   Δh_carry = Δh (1 - z) + Δ(r h) r + U_z' Δa_z + U_r' Δa_r;   dP[t] = (Δa_z, Δa_r, Δa_h),  S[t] = (h_{t-1}, r h_{t-1})
template <int NT>
__global__ void __launch_bounds__(256) tgcn_bwd_kernel(const float *__restrict__ dy, const float *__restrict__ y,
                                                       const float *__restrict__ gates, const float *__restrict__ Uzr,
                                                       const float *__restrict__ Uh, const float *__restrict__ h0, int64_t h0_stride,
                                                       float *__restrict__ dP, float *__restrict__ S, float *__restrict__ dh0, int64_t N,
                                                       int T, int out) {
    extern __shared__ f32x4 img[];
    tg_fill<true>(img, Uzr, Uh, out, NT, tg_nlds<NT>());
    __syncthreads();
    const int lane = threadIdx.x & 63, n = lane & 15, q = lane >> 4;
    const int64_t node = ((int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * 16 + n;
    const bool valid = node < N;
    if (((int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * 16 >= N) return;
    const int64_t D3 = 3 * (int64_t)out;
    const f32x4 zero4 = {0.0f, 0.0f, 0.0f, 0.0f};
    f32x4 dh[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) dh[j] = zero4;
    for (int t = T - 1; t >= 0; --t) {
        const float *gt = gates + (node * T + t) * D3;
        const float *dyt = dy + (node * T + t) * out;
        const float *hpp = t > 0 ? y + (node * T + t - 1) * out : (h0 ? h0 + node * h0_stride : nullptr);
        float *dPt = dP + (node * T + t) * D3;
        float *St = S ? S + (node * T + t) * 2 * (int64_t)out : nullptr;
        f32x4 daz[NT], dah[NT];
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const int c0 = 16 * j + 4 * q;
            const f32x4 z = valid ? tg_load4(gt, c0, out) : zero4;
            const f32x4 ht = valid ? tg_load4(gt + 2 * out, c0, out) : zero4;
            const f32x4 g = valid ? tg_load4(dyt, c0, out) : zero4;
            const f32x4 hp = (valid && hpp) ? tg_load4(hpp, c0, out) : zero4;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float d = g[i] + dh[j][i];
                dah[j][i] = (d * z[i]) * (1.0f - ht[i] * ht[i]);
                daz[j][i] = (d * (ht[i] - hp[i])) * (z[i] * (1.0f - z[i]));
                dh[j][i] = d * (1.0f - z[i]);
            }
            if (valid) {
                tg_store4(dPt, c0, out, daz[j]);
                tg_store4(dPt + 2 * out, c0, out, dah[j]);
            }
        }
        f32x4 drh[NT];
#pragma unroll
        for (int j = 0; j < NT; ++j) drh[j] = zero4;
        tg_prod<NT, NT, true>(drh, dah, img, Uzr, Uh, out, 2 * NT * NT, lane);
        // r and h_{t-1} read again (L1 / L2 hits) rather than held across the product
        f32x4 dar[NT];
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const int c0 = 16 * j + 4 * q;
            const f32x4 r = valid ? tg_load4(gt + out, c0, out) : zero4;
            const f32x4 hp = (valid && hpp) ? tg_load4(hpp, c0, out) : zero4;
            f32x4 rhp;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                dar[j][i] = (drh[j][i] * hp[i]) * (r[i] * (1.0f - r[i]));
                dh[j][i] = dh[j][i] + drh[j][i] * r[i];
                rhp[i] = r[i] * hp[i];
            }
            if (valid) {
                tg_store4(dPt + out, c0, out, dar[j]);
                if (St) {
                    tg_store4(St, c0, out, hp);
                    tg_store4(St + out, c0, out, rhp);
                }
            }
        }
        tg_prod<NT, NT, true>(dh, daz, img, Uzr, Uh, out, 0, lane);
        tg_prod<NT, NT, true>(dh, dar, img, Uzr, Uh, out, NT * NT, lane);
    }
    if (valid && dh0) {
#pragma unroll
        for (int j = 0; j < NT; ++j) tg_store4(dh0 + node * out, 16 * j + 4 * q, out, dh[j]);
    }
}

// ---- the per-step path's pointwise halves (a = the dense product of the step, [N][2D] or [N][D], contiguous) -----------------
// forward phase 0: z, r = σ(P_zr[t] + a);  gates[t] <- z, r;  rh = r .* h
// forward phase 1: h~ = tanh(P_h[t] + a);  gates[t] <- h~;  h' = (1 - z) h + z h~ -> y[t] and hout (contiguous)
__global__ void __launch_bounds__(256) tgcn_step_kernel(int phase, const float *__restrict__ P, const float *__restrict__ a,
                                                        const float *__restrict__ h, int64_t ldh, float *__restrict__ gates,
                                                        float *__restrict__ hout, float *__restrict__ y, int64_t N, int T, int t, int D) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= N * D) return;
    const int64_t n = idx / D;
    const int d = (int)(idx - n * D);
    const int64_t row = (n * T + t) * 3 * (int64_t)D;
    const float hv = h ? h[n * ldh + d] : 0.0f;
    if (phase == 0) {
        const float z = tg_sigmoid(P[row + d] + a[n * 2 * D + d]);
        const float r = tg_sigmoid(P[row + D + d] + a[n * 2 * D + D + d]);
        gates[row + d] = z;
        gates[row + D + d] = r;
        hout[idx] = r * hv;
    } else {
        const float ht = tanhf(P[row + 2 * D + d] + a[idx]);
        const float z = gates[row + d];
        gates[row + 2 * D + d] = ht;
        const float hn = (1.0f - z) * hv + z * ht;
        hout[idx] = hn;
        y[(n * T + t) * D + d] = hn;
    }
}

// backward phase 0: Δh = dy[t] + carry;  Δa_h, Δa_z -> dP[t] and the contiguous operands dah [N][D], dzr[:, 0:D];  part = Δh (1 - z)
// backward phase 1: (drh = U_h' Δa_h by the caller)  Δa_r -> dP[t], dzr[:, D:2D];  part += drh r;  S[t] = (h_{t-1}, r h_{t-1})
__global__ void __launch_bounds__(256) tgcn_step_grad_kernel(int phase, const float *__restrict__ dy, const float *__restrict__ carry,
                                                             const float *__restrict__ gates, const float *__restrict__ h, int64_t ldh,
                                                             const float *__restrict__ drh, float *__restrict__ dP, float *__restrict__ dah,
                                                             float *__restrict__ dzr, float *__restrict__ part, float *__restrict__ S,
                                                             int64_t N, int T, int t, int D) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= N * D) return;
    const int64_t n = idx / D;
    const int d = (int)(idx - n * D);
    const int64_t row = (n * T + t) * 3 * (int64_t)D;
    const float hp = h ? h[n * ldh + d] : 0.0f;
    const float z = gates[row + d], r = gates[row + D + d];
    if (phase == 0) {
        const float ht = gates[row + 2 * D + d];
        const float g = dy[(n * T + t) * D + d] + (carry ? carry[idx] : 0.0f);
        const float ah = (g * z) * (1.0f - ht * ht);
        const float az = (g * (ht - hp)) * (z * (1.0f - z));
        dP[row + d] = az;
        dP[row + 2 * D + d] = ah;
        dah[idx] = ah;
        dzr[n * 2 * D + d] = az;
        part[idx] = g * (1.0f - z);
    } else {
        const float ar = (drh[idx] * hp) * (r * (1.0f - r));
        dP[row + D + d] = ar;
        dzr[n * 2 * D + D + d] = ar;
        part[idx] = part[idx] + drh[idx] * r;
        if (S) {
            S[(n * T + t) * 2 * (int64_t)D + d] = hp;
            S[(n * T + t) * 2 * (int64_t)D + D + d] = r * hp;
        }
    }
}

template <int NT>
int launch_fwd(const float *P, const float *Uzr, const float *Uh, const float *h0, int64_t h0_stride, float *y, float *gates, int64_t N,
               int T, int out, hipStream_t stream) {
    GNNMP_LDS_OPTIN("tgcn_fwd_kernel", &tgcn_fwd_kernel<NT>);
    constexpr int nlds = tg_nlds<NT>();
    // four waves (64 nodes) a block, one block per CU (the U image takes the LDS); 256 threads let a wave use AGPRs beside its 256 VGPRs
    constexpr int wpb = 4;
    const int64_t blocks = ((N + 15) / 16 + wpb - 1) / wpb;
    tgcn_fwd_kernel<NT><<<(unsigned)blocks, 64 * wpb, nlds * 1024, stream>>>(P, Uzr, Uh, h0, h0_stride, y, gates, N, T, out);
    GNNMP_LAUNCH_CHECK("tgcn_fwd_kernel");
    return GNNMP_OK;
}

template <int NT>
int launch_bwd(const float *dy, const float *y, const float *gates, const float *Uzr, const float *Uh, const float *h0, int64_t h0_stride,
               float *dP, float *S, float *dh0, int64_t N, int T, int out, hipStream_t stream) {
    GNNMP_LDS_OPTIN("tgcn_bwd_kernel", &tgcn_bwd_kernel<NT>);
    constexpr int nlds = tg_nlds<NT>();
    // four waves (64 nodes) a block, one block per CU (the U image takes the LDS); 256 threads let a wave use AGPRs beside its 256 VGPRs
    constexpr int wpb = 4;
    const int64_t blocks = ((N + 15) / 16 + wpb - 1) / wpb;
    tgcn_bwd_kernel<NT><<<(unsigned)blocks, 64 * wpb, nlds * 1024, stream>>>(dy, y, gates, Uzr, Uh, h0, h0_stride, dP, S, dh0, N, T, out);
    GNNMP_LAUNCH_CHECK("tgcn_bwd_kernel");
    return GNNMP_OK;
}

int check_sizes(const char *what, int64_t N, int64_t T, int64_t out, int64_t h0_stride, int64_t max_out) {
    if (N < 0 || T < 1 || out < 1 || out > max_out || N * T > ((int64_t)1 << 40) || T > (1 << 20))
        return fail(GNNMP_EINVAL, "%s: bad size (N = %lld, T = %lld, out = %lld; 1 <= out <= %lld)", what, (long long)N, (long long)T,
                    (long long)out, (long long)max_out);
    if (h0_stride != 0 && h0_stride != out)
        return fail(GNNMP_EINVAL, "%s: h0_stride must be 0 (one state for every node) or out", what);
    return GNNMP_OK;
}

}  // namespace
}  // namespace gnnmp

using namespace gnnmp;

extern "C" {

int gnnmp_tgcn_recurrence_f32(const float *P, const float *U_zr, const float *U_h, const float *h0, int64_t h0_stride, float *y,
                              float *gates, int64_t N, int64_t T, int64_t out, gnnmp_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    int rc = check_sizes("tgcn_recurrence", N, T, out, h0_stride, TGCN_MAX_OUT);
    if (rc != GNNMP_OK) return rc;
    if (N == 0) return GNNMP_OK;
    if (!P || !U_zr || !U_h || !y) return fail(GNNMP_EINVAL, "tgcn_recurrence: null pointer");
    switch ((out + 15) / 16) {
        case 1: return launch_fwd<1>(P, U_zr, U_h, h0, h0_stride, y, gates, N, (int)T, (int)out, stream);
        case 2: return launch_fwd<2>(P, U_zr, U_h, h0, h0_stride, y, gates, N, (int)T, (int)out, stream);
        case 3: return launch_fwd<3>(P, U_zr, U_h, h0, h0_stride, y, gates, N, (int)T, (int)out, stream);
        case 4: return launch_fwd<4>(P, U_zr, U_h, h0, h0_stride, y, gates, N, (int)T, (int)out, stream);
        case 5: return launch_fwd<5>(P, U_zr, U_h, h0, h0_stride, y, gates, N, (int)T, (int)out, stream);
        case 6: return launch_fwd<6>(P, U_zr, U_h, h0, h0_stride, y, gates, N, (int)T, (int)out, stream);
        case 7: return launch_fwd<7>(P, U_zr, U_h, h0, h0_stride, y, gates, N, (int)T, (int)out, stream);
        default: return launch_fwd<8>(P, U_zr, U_h, h0, h0_stride, y, gates, N, (int)T, (int)out, stream);
    }
}

int gnnmp_tgcn_recurrence_grad_f32(const float *dy, const float *y, const float *gates, const float *U_zr, const float *U_h,
                                   const float *h0, int64_t h0_stride, float *dP, float *S, float *dh0, int64_t N, int64_t T,
                                   int64_t out, gnnmp_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    int rc = check_sizes("tgcn_recurrence_grad", N, T, out, h0_stride, TGCN_MAX_OUT);
    if (rc != GNNMP_OK) return rc;
    if (N == 0) return GNNMP_OK;
    if (!dy || !y || !gates || !U_zr || !U_h || !dP) return fail(GNNMP_EINVAL, "tgcn_recurrence_grad: null pointer");
    switch ((out + 15) / 16) {
        case 1: return launch_bwd<1>(dy, y, gates, U_zr, U_h, h0, h0_stride, dP, S, dh0, N, (int)T, (int)out, stream);
        case 2: return launch_bwd<2>(dy, y, gates, U_zr, U_h, h0, h0_stride, dP, S, dh0, N, (int)T, (int)out, stream);
        case 3: return launch_bwd<3>(dy, y, gates, U_zr, U_h, h0, h0_stride, dP, S, dh0, N, (int)T, (int)out, stream);
        case 4: return launch_bwd<4>(dy, y, gates, U_zr, U_h, h0, h0_stride, dP, S, dh0, N, (int)T, (int)out, stream);
        case 5: return launch_bwd<5>(dy, y, gates, U_zr, U_h, h0, h0_stride, dP, S, dh0, N, (int)T, (int)out, stream);
        case 6: return launch_bwd<6>(dy, y, gates, U_zr, U_h, h0, h0_stride, dP, S, dh0, N, (int)T, (int)out, stream);
        case 7: return launch_bwd<7>(dy, y, gates, U_zr, U_h, h0, h0_stride, dP, S, dh0, N, (int)T, (int)out, stream);
        default: return launch_bwd<8>(dy, y, gates, U_zr, U_h, h0, h0_stride, dP, S, dh0, N, (int)T, (int)out, stream);
    }
}

int gnnmp_tgcn_step_f32(int phase, const float *P, const float *a, const float *h, int64_t ldh, float *gates, float *hout, float *y,
                        int64_t N, int64_t T, int64_t t, int64_t D, gnnmp_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (phase != 0 && phase != 1) return fail(GNNMP_EINVAL, "tgcn_step: bad phase %d", phase);
    int rc = check_sizes("tgcn_step", N, T, D, 0, (int64_t)1 << 20);
    if (rc != GNNMP_OK) return rc;
    if (t < 0 || t >= T || (h && ldh < D)) return fail(GNNMP_EINVAL, "tgcn_step: bad step / state stride");
    if (N == 0) return GNNMP_OK;
    if (!P || !a || !gates || !hout || (phase == 1 && !y)) return fail(GNNMP_EINVAL, "tgcn_step: null pointer");
    tgcn_step_kernel<<<(unsigned)((N * D + 255) / 256), 256, 0, stream>>>(phase, P, a, h, ldh, gates, hout, y, N, (int)T, (int)t, (int)D);
    GNNMP_LAUNCH_CHECK("tgcn_step_kernel");
    return GNNMP_OK;
}

int gnnmp_tgcn_step_grad_f32(int phase, const float *dy, const float *carry, const float *gates, const float *h, int64_t ldh,
                             const float *drh, float *dP, float *dah, float *dzr, float *part, float *S, int64_t N, int64_t T, int64_t t,
                             int64_t D, gnnmp_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (phase != 0 && phase != 1) return fail(GNNMP_EINVAL, "tgcn_step_grad: bad phase %d", phase);
    int rc = check_sizes("tgcn_step_grad", N, T, D, 0, (int64_t)1 << 20);
    if (rc != GNNMP_OK) return rc;
    if (t < 0 || t >= T || (h && ldh < D)) return fail(GNNMP_EINVAL, "tgcn_step_grad: bad step / state stride");
    if (N == 0) return GNNMP_OK;
    if (!gates || !dP || !dzr || !part || (phase == 0 && (!dy || !dah)) || (phase == 1 && !drh))
        return fail(GNNMP_EINVAL, "tgcn_step_grad: null pointer");
    tgcn_step_grad_kernel<<<(unsigned)((N * D + 255) / 256), 256, 0, stream>>>(phase, dy, carry, gates, h, ldh, drh, dP, dah, dzr, part, S, N,
                                                                               (int)T, (int)t, (int)D);
    GNNMP_LAUNCH_CHECK("tgcn_step_grad_kernel");
    return GNNMP_OK;
}

}  // extern "C"
