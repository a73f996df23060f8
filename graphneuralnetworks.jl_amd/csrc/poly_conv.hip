// poly_conv.hip — the two kernels the last four convolution layers need to train on libgnnmp (include/gnnmp.h states the arithmetic).
//   poly_hop_kernel            one step of a three-term recurrence over a plan, Z_k = α ÃZ_{k-1} + β Z_{k-1} + γ Z_{k-2} (+ addend), in ONE
//                              launch: the order k >= 2 of cheb_conv (GNNlib/src/layers/conv.jl:83-98), the `2 * step - T0` of d_conv
//                              (conv.jl:696-724) and — over the transposed plan, with the addend — their pullbacks, which are the same
//                              recurrence run backwards (Clenshaw): B_k = G_k + 2 L̃ᵀB_{k+1} - B_{k+2}.  A lane group owns destination i and
//                              walks its row whole; the per-slot factor and the fold are reduce_range<SCALED>'s expressions (csr_reduce.h),
//                              so the aggregate has gnnmp_propagate_slots_f32's bits on every row that export does not split.
//   gru_pointwise_grad_kernel  pullback of gru_pointwise_kernel (leaf.hip), the cell of gated_graph_conv (conv.jl:218-233): r, z, h~ by the
//                              forward's expressions, then the chain rule term by term.  Elementwise.
// The hop is a whole-row walk on the shared pieces and conventions of slotwalk.h (no atomics, every output written once, a hub row by one
// lane group: correct, slow).  It reads col only, never eid: a plan with self loops of its own is fine.
//
// The epilogue's products and sums are separate roundings in the order of the header: this file is compiled with -ffp-contract=off like
// the rest of the library (Makefile), nothing here is an fmaf.
// Registers: U = 4 slots in flight, one gathered vector a slot — 16 VGPRs of loads with 16-byte lanes.  The compiler's resource report
// (LABNOTES.md) shows no scratch for any instance.
#include "csr_reduce.h"
#include "launch.h"

namespace gnnmp {

struct PolyHopArgs {
    PlanRows rows;               // the plan or the transposed plan, whole rows (plan_rows_whole)
    RowGeom geom;
    const float *z;              // [n_src][D]
    const float *w_slot;         // [n_total] or null, read by the SCALED instances only
    const float *ss_slot;        // [n_total] or null, ditto
    const float *sd;             // [n_dst] or null
    const float *self_, *prev, *add;      // [n_dst][D] or null; prev and add may be out (no __restrict__ anywhere here)
    float alpha, beta, gamma;
    float *out;                  // [n_dst][D]
    int D;
};

template <int VEC, int U, bool SCALED>
__global__ void __launch_bounds__(256) poly_hop_kernel(const PolyHopArgs a) {
    RowLane w;
    if (!decode_row_lane<VEC>(a.rows, a.geom, a.D, w)) return;
    const int f0 = w.f0;
    const bool active = w.active;
    const int64_t ld = a.D;
    float acc[VEC];
#pragma unroll
    for (int q = 0; q < VEC; ++q) acc[q] = 0.0f;
    for (uint32_t base = w.beg; base < w.end; base += w.G) {
        const Slots s = load_slots<true, false>(a.rows.col, a.rows.eid, base, w.end, w.lig, w.G);
        float wv = 1.0f, sv = 1.0f;
        if (SCALED) {
            const uint32_t p = base + w.lig;
            if (p < w.end) {
                if (a.w_slot) wv = a.w_slot[p];
                if (a.ss_slot) sv = a.ss_slot[p];
            }
        }
        for (int j = 0; j < s.n; j += U) {
            float v[U][VEC], wj[SCALED ? U : 1], sj[SCALED ? U : 1];
            int cjs[U];
            uint32_t ejs[U];
            bcast_slots<U, true, false>(s, w.gbase, j, cjs, ejs);
            if (SCALED) {
                bcast_word<SCALED ? U : 1>(wv, s.n, w.gbase, j, wj);
                bcast_word<SCALED ? U : 1>(sv, s.n, w.gbase, j, sj);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) load_or_zero<VEC>(active, a.z + (int64_t)cjs[u] * ld + f0, v[u]);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (j + u < s.n) {
#pragma unroll
                    for (int q = 0; q < VEC; ++q) {
                        float t = v[u][q];
                        if (SCALED) {      // reduce_range<SCALED>: the source factor, then the weight, each rounded
                            t = t * sj[SCALED ? u : 0];
                            t = wj[SCALED ? u : 0] * t;
                        }
                        acc[q] = acc[q] + t;
                    }
                }
            }
        }
    }
    if (!active) return;
    if (a.sd) {
        const float sc = a.sd[w.row];
#pragma unroll
        for (int q = 0; q < VEC; ++q) acc[q] = acc[q] * sc;
    }
    const int64_t o = (int64_t)w.row * ld + f0;
    float r[VEC], t[VEC];
#pragma unroll
    for (int q = 0; q < VEC; ++q) r[q] = a.alpha * acc[q];
    if (a.self_) {
        Vec<VEC>::load(a.self_ + o, t);
#pragma unroll
        for (int q = 0; q < VEC; ++q) r[q] = r[q] + a.beta * t[q];
    }
    if (a.prev) {
        Vec<VEC>::load(a.prev + o, t);
#pragma unroll
        for (int q = 0; q < VEC; ++q) r[q] = r[q] + a.gamma * t[q];
    }
    if (a.add) {
        Vec<VEC>::load(a.add + o, t);
#pragma unroll
        for (int q = 0; q < VEC; ++q) r[q] = r[q] + t[q];
    }
    Vec<VEC>::store(a.out + o, r);      // after every load of this lane: out may be prev or add
}

// dh may be base: each element is read, then written, by one thread (no __restrict__ on the two)
__global__ void __launch_bounds__(256) gru_pointwise_grad_kernel(const float *__restrict__ gx, const float *__restrict__ gh,
                                                                 const float *__restrict__ b, const float *__restrict__ h,
                                                                 const float *__restrict__ dout, const float *base,
                                                                 float *__restrict__ dgx, float *__restrict__ dgh, float *dh, int64_t N,
                                                                 int D) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N * D) return;
    const int64_t n = i / D;
    const int d = (int)(i - n * D);
    const int64_t o = n * 3 * D + d;
    // the forward's expressions (gru_pointwise_kernel)
    const float br = b ? b[d] : 0.0f, bz = b ? b[D + d] : 0.0f, bn = b ? b[2 * D + d] : 0.0f;
    const float xr = gx[o] + gh[o] + br, xz = gx[o + D] + gh[o + D] + bz;
    const float tr = expf(-fabsf(xr)), tz = expf(-fabsf(xz));
    const float r = xr >= 0.0f ? 1.0f / (1.0f + tr) : tr / (1.0f + tr);
    const float z = xz >= 0.0f ? 1.0f / (1.0f + tz) : tz / (1.0f + tz);
    const float ghn = gh[o + 2 * (int64_t)D];
    const float c = tanhf(gx[o + 2 * (int64_t)D] + r * ghn + bn);
    // h' = (1 - z) c + z h
    const float dv = dout[i];
    const float dhv = dv * z;
    const float dz = (dv * (h[i] - c)) * (z * (1.0f - z));
    const float dn = (dv * (1.0f - z)) * (1.0f - c * c);
    const float dr = (dn * ghn) * (r * (1.0f - r));
    dgx[o] = dr;
    dgx[o + D] = dz;
    dgx[o + 2 * (int64_t)D] = dn;
    dgh[o] = dr;
    dgh[o + D] = dz;
    dgh[o + 2 * (int64_t)D] = dn * r;
    dh[i] = base ? base[i] + dhv : dhv;
}

}  // namespace gnnmp

using namespace gnnmp;

extern "C" int gnnmp_poly_hop_f32(const gnnmp_graph_t *plan, const gnnmp_poly_hop_t *job, int64_t D, gnnmp_stream_t stream) {
    const char *who = "poly_hop";
    if (!plan) return fail(GNNMP_EINVAL, "%s: null plan", who);
    if (!job) return fail(GNNMP_EINVAL, "%s: null job", who);
    if (!job->z) return fail(GNNMP_EINVAL, "%s: null z", who);
    if (!job->out) return fail(GNNMP_EINVAL, "%s: null out", who);
    if (D < 1 || D > (1 << 19)) return fail(GNNMP_EINVAL, "%s: bad D %lld (1 .. 2^19)", who, (long long)D);
    if (job->out == job->z) return fail(GNNMP_EINVAL, "%s: out aliases z (other lanes gather it)", who);
    if (job->out == job->self) return fail(GNNMP_EINVAL, "%s: out aliases self", who);
    if (job->beta != 0.0f && !job->self) return fail(GNNMP_EINVAL, "%s: beta != 0 with a null self", who);
    if (job->gamma != 0.0f && !job->prev) return fail(GNNMP_EINVAL, "%s: gamma != 0 with a null prev", who);
    if (plan->n_dst == 0) return GNNMP_OK;
    PolyHopArgs a = {};
    a.rows = plan_rows_whole(plan);
    a.z = job->z;
    a.w_slot = job->w_slot;
    a.ss_slot = job->ss_slot;
    a.sd = job->scale_dst;
    a.self_ = job->self;
    a.prev = job->prev;
    a.add = job->add;
    a.alpha = job->alpha;
    a.beta = job->beta;
    a.gamma = job->gamma;
    a.out = job->out;
    a.D = (int)D;
    dim3 grid;
    const int vec = row_walk_geom(who, a.rows, D, 0, {job->z, job->self, job->prev, job->add, job->out}, a.geom, grid);
    if (vec < 0) return vec;
    const bool scaled = job->w_slot || job->ss_slot;
    with_vec(vec, [&](auto V) {
        if (scaled)
            poly_hop_kernel<decltype(V)::value, 4, true><<<grid, 256, 0, (hipStream_t)stream>>>(a);
        else
            poly_hop_kernel<decltype(V)::value, 4, false><<<grid, 256, 0, (hipStream_t)stream>>>(a);
    });
    GNNMP_LAUNCH_CHECK("poly_hop_kernel");
    return GNNMP_OK;
}

extern "C" int gnnmp_gru_pointwise_grad_f32(const gnnmp_gru_grad_t *job, int64_t N, int64_t D, gnnmp_stream_t stream) {
    const char *who = "gru_pointwise_grad";
    if (!job) return fail(GNNMP_EINVAL, "%s: null job", who);
    if (N < 0) return fail(GNNMP_EINVAL, "%s: negative N %lld", who, (long long)N);
    if (D < 1 || D > (1 << 20)) return fail(GNNMP_EINVAL, "%s: bad D %lld (1 .. 2^20)", who, (long long)D);
    if (!job->gx || !job->gh || !job->h || !job->dout) return fail(GNNMP_EINVAL, "%s: null gx, gh, h or dout", who);
    if (!job->dgx || !job->dgh || !job->dh) return fail(GNNMP_EINVAL, "%s: null dgx, dgh or dh", who);
    if (N == 0) return GNNMP_OK;
    if ((N * D + 255) / 256 >= INT32_MAX) return fail(GNNMP_EUNSUPPORTED, "%s: N * D too large", who);
    gru_pointwise_grad_kernel<<<(unsigned)((N * D + 255) / 256), 256, 0, (hipStream_t)stream>>>(job->gx, job->gh, job->b, job->h, job->dout,
                                                                                                 job->base, job->dgx, job->dgh, job->dh, N,
                                                                                                 (int)D);
    GNNMP_LAUNCH_CHECK("gru_pointwise_grad_kernel");
    return GNNMP_OK;
}
