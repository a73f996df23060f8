// recurrent.hip — the node-local halves of the graph-convolutional recurrent cells (GraphNeuralNetworks/src/layers/temporalconv.jl):
// GConvGRUCell (:237-254) and DCGRUCell (:564-575) share one GRU cell, GConvLSTMCell (:416-437) is a peephole LSTM.  The spatial work of a
// step — the Chebyshev or diffusion basis of the state, built by gnnmp_poly_hop_ld_f32 into a panel [N][B D], and ONE dense product over
// that panel with the gate-stacked weights — is done by the caller; what is left is elementwise and lives here, forward and pullback
// (include/gnnmp.h states the arithmetic term by term).
//   gru_cell_kernel        phase 0: r, z = σ(P[t] + a) -> gates[t], r .* h -> block 0 of the panel the candidate's basis is built in
//                          phase 1: c = tanh(P_c[t] + a) -> gates[t], h' = (1 - z) c + z h -> y[n][t] and block 0 of the next step's panel
//   gru_cell_grad_kernel   phase 1, then phase 0, of the pullback; the carry arrives as up to two addends (the direct term `part` and the
//                          panel cotangent's block 0 after the Clenshaw recurrence)
//   lstm_cell_kernel       i, f, g, c', o, h' in one pass
//   lstm_cell_grad_kernel  its pullback in one pass, with the four peephole products as an optional output
// One thread an element; no atomics, every output element written once by one lane; a state may be [N][D] with a row stride, one vector
// for every node (stride 0) or NULL (zeros).  `rep`: DConv reads the state with TWO weight slices (one per direction), so its panel holds
// the state in blocks 0 and 1 — the forward writes hout `rep` times side by side, the pullback sums `rep` side-by-side cotangent blocks.
// σ and tanh are gru_pointwise_kernel's expressions (leaf.hip).  Compiled with -ffp-contract=off: no product and sum here is fused.
#include "common.h"

namespace gnnmp {

namespace {

__device__ __forceinline__ float rc_sigmoid(float x) {     // NNlib.σ: t = exp(-|x|); x >= 0 ? 1 / (1 + t) : t / (1 + t)
    const float t = expf(-fabsf(x));
    return x >= 0.0f ? 1.0f / (1.0f + t) : t / (1.0f + t);
}

struct GruCellArgs {
    const float *P, *a, *h;
    int64_t ldh;
    float *gates, *hout;
    int64_t ldhout;
    int rep;
    float *y;
    int64_t N;
    int T, t, D;
};

__global__ void __launch_bounds__(256) gru_cell_kernel(int phase, const GruCellArgs k) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= k.N * k.D) return;
    const int D = k.D;
    const int64_t n = idx / D;
    const int d = (int)(idx - n * D);
    const int64_t row = (n * k.T + k.t) * 3 * (int64_t)D;
    const float hv = k.h ? k.h[n * k.ldh + d] : 0.0f;
    float o;
    if (phase == 0) {
        const float r = rc_sigmoid(k.P[row + d] + k.a[n * 2 * D + d]);
        const float z = rc_sigmoid(k.P[row + D + d] + k.a[n * 2 * D + D + d]);
        k.gates[row + d] = r;
        k.gates[row + D + d] = z;
        o = r * hv;
    } else {
        const float c = tanhf(k.P[row + 2 * (int64_t)D + d] + k.a[idx]);
        const float z = k.gates[row + D + d];
        k.gates[row + 2 * (int64_t)D + d] = c;
        o = (1.0f - z) * c + z * hv;
        k.y[(n * k.T + k.t) * D + d] = o;
    }
    if (k.hout) {
        for (int j = 0; j < k.rep; ++j) k.hout[n * k.ldhout + (int64_t)j * D + d] = o;
    }
}

struct GruCellGradArgs {
    const float *dy, *carry, *carry2;
    int64_t ldc2;
    const float *gates, *h;
    int64_t ldh;
    const float *drh;
    int64_t lddrh;
    int rep;
    float *dP, *dac, *darz, *part;
    int64_t N;
    int T, t, D;
};

__global__ void __launch_bounds__(256) gru_cell_grad_kernel(int phase, const GruCellGradArgs k) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= k.N * k.D) return;
    const int D = k.D;
    const int64_t n = idx / D;
    const int d = (int)(idx - n * D);
    const int64_t row = (n * k.T + k.t) * 3 * (int64_t)D;
    const float hv = k.h ? k.h[n * k.ldh + d] : 0.0f;
    const float r = k.gates[row + d], z = k.gates[row + D + d];
    if (phase == 1) {
        const float c = k.gates[row + 2 * (int64_t)D + d];
        float g = k.dy[(n * k.T + k.t) * D + d];
        if (k.carry) g = g + k.carry[idx];
        if (k.carry2) {
            for (int j = 0; j < k.rep; ++j) g = g + k.carry2[n * k.ldc2 + (int64_t)j * D + d];
        }
        const float dc = (g * (1.0f - z)) * (1.0f - c * c);
        const float dz = (g * (hv - c)) * (z * (1.0f - z));
        k.dP[row + 2 * (int64_t)D + d] = dc;
        k.dP[row + D + d] = dz;
        k.dac[idx] = dc;
        k.darz[n * 2 * D + D + d] = dz;
        k.part[idx] = g * z;
    } else {
        float q = k.drh[n * k.lddrh + d];
        for (int j = 1; j < k.rep; ++j) q = q + k.drh[n * k.lddrh + (int64_t)j * D + d];
        const float dr = (q * hv) * (r * (1.0f - r));
        k.dP[row + d] = dr;
        k.darz[n * 2 * D + d] = dr;
        k.part[idx] = k.part[idx] + q * r;
    }
}

struct LstmCellArgs {
    const float *P, *a, *w, *c;
    int64_t ldc;
    float *gates, *cnew, *hout;
    int64_t ldhout;
    float *y;
    int64_t N;
    int T, t, D;
};

__global__ void __launch_bounds__(256) lstm_cell_kernel(const LstmCellArgs k) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= k.N * k.D) return;
    const int D = k.D;
    const int64_t n = idx / D;
    const int d = (int)(idx - n * D);
    const int64_t row = (n * k.T + k.t) * 4 * (int64_t)D, ar = n * 4 * (int64_t)D;
    const float cv = k.c ? k.c[n * k.ldc + d] : 0.0f;
    const float wi = k.w[d], wf = k.w[D + d], wc = k.w[2 * (int64_t)D + d], wo = k.w[3 * (int64_t)D + d];
    const float i = rc_sigmoid(k.P[row + d] + k.a[ar + d] + wi * cv);
    const float f = rc_sigmoid(k.P[row + D + d] + k.a[ar + D + d] + wf * cv);
    const float g = tanhf(k.P[row + 2 * (int64_t)D + d] + k.a[ar + 2 * (int64_t)D + d] + wc * cv);
    const float cn = f * cv + i * g;
    const float o = rc_sigmoid(k.P[row + 3 * (int64_t)D + d] + k.a[ar + 3 * (int64_t)D + d] + wo * cn);
    const float hn = o * tanhf(cn);
    k.gates[row + d] = i;
    k.gates[row + D + d] = f;
    k.gates[row + 2 * (int64_t)D + d] = g;
    k.gates[row + 3 * (int64_t)D + d] = o;
    k.cnew[(n * k.T + k.t) * D + d] = cn;
    k.y[(n * k.T + k.t) * D + d] = hn;
    if (k.hout) k.hout[n * k.ldhout + d] = hn;
}

struct LstmCellGradArgs {
    const float *dy, *carry_h;
    int64_t ldch;
    const float *carry_c, *gates, *w, *c;
    int64_t ldc;
    const float *cnew;
    float *dP, *da, *dc, *peep;
    int64_t N;
    int T, t, D;
};

__global__ void __launch_bounds__(256) lstm_cell_grad_kernel(const LstmCellGradArgs k) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= k.N * k.D) return;
    const int D = k.D;
    const int64_t n = idx / D;
    const int d = (int)(idx - n * D);
    const int64_t row = (n * k.T + k.t) * 4 * (int64_t)D, ar = n * 4 * (int64_t)D;
    const float cv = k.c ? k.c[n * k.ldc + d] : 0.0f;
    const float cn = k.cnew[(n * k.T + k.t) * D + d];
    const float wi = k.w[d], wf = k.w[D + d], wc = k.w[2 * (int64_t)D + d], wo = k.w[3 * (int64_t)D + d];
    const float i = k.gates[row + d], f = k.gates[row + D + d], g = k.gates[row + 2 * (int64_t)D + d], o = k.gates[row + 3 * (int64_t)D + d];
    float dh = k.dy[(n * k.T + k.t) * D + d];
    if (k.carry_h) dh = dh + k.carry_h[n * k.ldch + d];
    const float th = tanhf(cn);
    const float d_o = (dh * th) * (o * (1.0f - o));
    float dcn = (dh * o) * (1.0f - th * th);
    if (k.carry_c) dcn = dcn + k.carry_c[idx];
    dcn = dcn + d_o * wo;
    const float d_i = (dcn * g) * (i * (1.0f - i));
    const float d_f = (dcn * cv) * (f * (1.0f - f));
    const float d_g = (dcn * i) * (1.0f - g * g);
    k.dP[row + d] = d_i;
    k.dP[row + D + d] = d_f;
    k.dP[row + 2 * (int64_t)D + d] = d_g;
    k.dP[row + 3 * (int64_t)D + d] = d_o;
    k.da[ar + d] = d_i;
    k.da[ar + D + d] = d_f;
    k.da[ar + 2 * (int64_t)D + d] = d_g;
    k.da[ar + 3 * (int64_t)D + d] = d_o;
    k.dc[idx] = dcn * f + d_i * wi + d_f * wf + d_g * wc;
    if (k.peep) {
        k.peep[row + d] = d_i * cv;
        k.peep[row + D + d] = d_f * cv;
        k.peep[row + 2 * (int64_t)D + d] = d_g * cv;
        k.peep[row + 3 * (int64_t)D + d] = d_o * cn;
    }
}

// N, T, t, D of a step call; the element count must fit a grid of 256-thread blocks
int check_step(const char *who, int64_t N, int64_t T, int64_t t, int64_t D) {
    if (N < 0) return fail(GNNMP_EINVAL, "%s: negative N %lld", who, (long long)N);
    if (D < 1 || D > (1 << 20)) return fail(GNNMP_EINVAL, "%s: bad D %lld (1 .. 2^20)", who, (long long)D);
    if (T < 1 || T > (1 << 20)) return fail(GNNMP_EINVAL, "%s: bad T %lld (1 .. 2^20)", who, (long long)T);
    if (t < 0 || t >= T) return fail(GNNMP_EINVAL, "%s: step %lld outside [0, T)", who, (long long)t);
    if (N > ((int64_t)1 << 40) / T) return fail(GNNMP_EINVAL, "%s: N * T above 2^40", who);
    return GNNMP_OK;
}
int check_state(const char *who, const char *what, const void *p, int64_t ld, int64_t D) {
    if (p && ld != 0 && ld < D) return fail(GNNMP_EINVAL, "%s: stride of %s is %lld: 0 (one vector) or at least D", who, what, (long long)ld);
    return GNNMP_OK;
}
int check_grid(const char *who, int64_t N, int64_t D, unsigned &blocks) {
    const int64_t b = (N * D + 255) / 256;
    if (b >= INT32_MAX) return fail(GNNMP_EUNSUPPORTED, "%s: N * D too large", who);
    blocks = (unsigned)b;
    return GNNMP_OK;
}

}  // namespace
}  // namespace gnnmp

using namespace gnnmp;

extern "C" {

int gnnmp_gru_cell_f32(int phase, const gnnmp_gru_cell_t *job, int64_t N, int64_t T, int64_t t, int64_t D, gnnmp_stream_t stream) {
    const char *who = "gru_cell";
    if (!job) return fail(GNNMP_EINVAL, "%s: null job", who);
    if (phase != 0 && phase != 1) return fail(GNNMP_EINVAL, "%s: bad phase %d", who, phase);
    int rc = check_step(who, N, T, t, D);
    if (rc != GNNMP_OK) return rc;
    if (!job->P || !job->a || !job->gates) return fail(GNNMP_EINVAL, "%s: null P, a or gates", who);
    if (phase == 0 && !job->hout) return fail(GNNMP_EINVAL, "%s: null hout in phase 0", who);
    if (phase == 1 && !job->y) return fail(GNNMP_EINVAL, "%s: null y in phase 1", who);
    if ((rc = check_state(who, "h", job->h, job->ldh, D)) != GNNMP_OK) return rc;
    if (job->hout && (job->rep < 1 || job->rep > 2)) return fail(GNNMP_EINVAL, "%s: bad rep %d (1 or 2)", who, job->rep);
    if (job->hout && job->ldhout < (int64_t)job->rep * D) return fail(GNNMP_EINVAL, "%s: ldhout %lld below rep * D", who, (long long)job->ldhout);
    if (N == 0) return GNNMP_OK;
    unsigned blocks;
    if ((rc = check_grid(who, N, D, blocks)) != GNNMP_OK) return rc;
    GruCellArgs k = {job->P, job->a, job->h, job->ldh, job->gates, job->hout, job->ldhout, job->rep, job->y, N, (int)T, (int)t, (int)D};
    gru_cell_kernel<<<blocks, 256, 0, (hipStream_t)stream>>>(phase, k);
    GNNMP_LAUNCH_CHECK("gru_cell_kernel");
    return GNNMP_OK;
}

int gnnmp_gru_cell_grad_f32(int phase, const gnnmp_gru_cell_grad_t *job, int64_t N, int64_t T, int64_t t, int64_t D,
                            gnnmp_stream_t stream) {
    const char *who = "gru_cell_grad";
    if (!job) return fail(GNNMP_EINVAL, "%s: null job", who);
    if (phase != 0 && phase != 1) return fail(GNNMP_EINVAL, "%s: bad phase %d", who, phase);
    int rc = check_step(who, N, T, t, D);
    if (rc != GNNMP_OK) return rc;
    if (!job->gates || !job->dP || !job->darz || !job->part) return fail(GNNMP_EINVAL, "%s: null gates, dP, darz or part", who);
    if (phase == 1 && (!job->dy || !job->dac)) return fail(GNNMP_EINVAL, "%s: null dy or dac in phase 1", who);
    if (phase == 0 && !job->drh) return fail(GNNMP_EINVAL, "%s: null drh in phase 0", who);
    if ((rc = check_state(who, "h", job->h, job->ldh, D)) != GNNMP_OK) return rc;
    if (job->rep < 1 || job->rep > 2) return fail(GNNMP_EINVAL, "%s: bad rep %d (1 or 2)", who, job->rep);
    if (phase == 1 && job->carry2 && job->ldc2 < (int64_t)job->rep * D)
        return fail(GNNMP_EINVAL, "%s: ldc2 %lld below rep * D", who, (long long)job->ldc2);
    if (phase == 0 && job->lddrh < (int64_t)job->rep * D) return fail(GNNMP_EINVAL, "%s: lddrh %lld below rep * D", who, (long long)job->lddrh);
    if (N == 0) return GNNMP_OK;
    unsigned blocks;
    if ((rc = check_grid(who, N, D, blocks)) != GNNMP_OK) return rc;
    GruCellGradArgs k = {job->dy,  job->carry, job->carry2, job->ldc2, job->gates, job->h,    job->ldh, job->drh, job->lddrh,
                         job->rep, job->dP,    job->dac,    job->darz, job->part,  N,         (int)T,   (int)t,   (int)D};
    gru_cell_grad_kernel<<<blocks, 256, 0, (hipStream_t)stream>>>(phase, k);
    GNNMP_LAUNCH_CHECK("gru_cell_grad_kernel");
    return GNNMP_OK;
}

int gnnmp_lstm_cell_f32(const gnnmp_lstm_cell_t *job, int64_t N, int64_t T, int64_t t, int64_t D, gnnmp_stream_t stream) {
    const char *who = "lstm_cell";
    if (!job) return fail(GNNMP_EINVAL, "%s: null job", who);
    int rc = check_step(who, N, T, t, D);
    if (rc != GNNMP_OK) return rc;
    if (!job->P || !job->a || !job->w) return fail(GNNMP_EINVAL, "%s: null P, a or w", who);
    if (!job->gates || !job->cnew || !job->y) return fail(GNNMP_EINVAL, "%s: null gates, cnew or y", who);
    if ((rc = check_state(who, "c", job->c, job->ldc, D)) != GNNMP_OK) return rc;
    if (job->hout && job->ldhout < D) return fail(GNNMP_EINVAL, "%s: ldhout %lld below D", who, (long long)job->ldhout);
    if (N == 0) return GNNMP_OK;
    unsigned blocks;
    if ((rc = check_grid(who, N, D, blocks)) != GNNMP_OK) return rc;
    LstmCellArgs k = {job->P, job->a, job->w, job->c, job->ldc, job->gates, job->cnew, job->hout, job->ldhout, job->y, N, (int)T, (int)t, (int)D};
    lstm_cell_kernel<<<blocks, 256, 0, (hipStream_t)stream>>>(k);
    GNNMP_LAUNCH_CHECK("lstm_cell_kernel");
    return GNNMP_OK;
}

int gnnmp_lstm_cell_grad_f32(const gnnmp_lstm_cell_grad_t *job, int64_t N, int64_t T, int64_t t, int64_t D, gnnmp_stream_t stream) {
    const char *who = "lstm_cell_grad";
    if (!job) return fail(GNNMP_EINVAL, "%s: null job", who);
    int rc = check_step(who, N, T, t, D);
    if (rc != GNNMP_OK) return rc;
    if (!job->dy || !job->gates || !job->w || !job->cnew) return fail(GNNMP_EINVAL, "%s: null dy, gates, w or cnew", who);
    if (!job->dP || !job->da || !job->dc) return fail(GNNMP_EINVAL, "%s: null dP, da or dc", who);
    if ((rc = check_state(who, "c", job->c, job->ldc, D)) != GNNMP_OK) return rc;
    if (job->carry_h && job->ldch < D) return fail(GNNMP_EINVAL, "%s: ldch %lld below D", who, (long long)job->ldch);
    if (N == 0) return GNNMP_OK;
    unsigned blocks;
    if ((rc = check_grid(who, N, D, blocks)) != GNNMP_OK) return rc;
    LstmCellGradArgs k = {job->dy, job->carry_h, job->ldch, job->carry_c, job->gates, job->w,  job->c, job->ldc, job->cnew,
                          job->dP, job->da,      job->dc,   job->peep,    N,          (int)T,  (int)t, (int)D};
    lstm_cell_grad_kernel<<<blocks, 256, 0, (hipStream_t)stream>>>(k);
    GNNMP_LAUNCH_CHECK("lstm_cell_grad_kernel");
    return GNNMP_OK;
}

}  // extern "C"
