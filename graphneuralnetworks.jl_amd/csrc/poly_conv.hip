// poly_conv.hip — the two kernels the last four convolution layers need to train on libgnnmp (include/gnnmp.h states the arithmetic).
//   poly_hop_kernel            one step of a three-term recurrence over a plan, Z_k = α ÃZ_{k-1} + β Z_{k-1} + γ Z_{k-2} (+ addend), in ONE
//                              launch: the order k >= 2 of cheb_conv (GNNlib/src/layers/conv.jl:83-98), the `2 * step - T0` of d_conv
//                              (conv.jl:696-724) and — over the transposed plan, with the addend — their pullbacks, which are the same
//                              recurrence run backwards (Clenshaw): B_k = G_k + 2 L̃ᵀB_{k+1} - B_{k+2}.  A lane group owns destination i and
//                              walks its row whole; the per-slot factor and the fold are reduce_range<SCALED>'s expressions (csr_reduce.h),
//                              so the aggregate has gnnmp_propagate_slots_f32's bits on every row that export does not split.
//   gru_pointwise_grad_kernel  pullback of gru_pointwise_kernel (leaf.hip), the cell of gated_graph_conv (conv.jl:218-233): r, z, h~ by the
//                              forward's expressions, then the chain rule term by term.  Elementwise.
// gnnmp_poly_hop_ld_f32 launches the SAME template with a row stride of its own for each of z, self, prev, add and out, so that the basis
// of a recurrent cell's state lands in the column blocks of one panel [N][B D] (gnnmp/layers_temporal.py); gnnmp_poly_hop_f32 passes D
// five times and keeps its bits.
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
    int64_t ldz, lds, ldp, lda, ldo;      // row strides in floats of z, self_, prev, add, out: all D for gnnmp_poly_hop_f32, a panel's for _ld
};

template <int VEC, int U, bool SCALED>
__global__ void __launch_bounds__(256) poly_hop_kernel(const PolyHopArgs a) {
    RowLane w;
    if (!decode_row_lane<VEC>(a.rows, a.geom, a.D, w)) return;
    const int f0 = w.f0;
    const bool active = w.active;
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
            for (int u = 0; u < U; ++u) load_or_zero<VEC>(active, a.z + (int64_t)cjs[u] * a.ldz + f0, v[u]);
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
    float r[VEC], t[VEC];
#pragma unroll
    for (int q = 0; q < VEC; ++q) r[q] = a.alpha * acc[q];
    if (a.self_) {
        Vec<VEC>::load(a.self_ + (int64_t)w.row * a.lds + f0, t);
#pragma unroll
        for (int q = 0; q < VEC; ++q) r[q] = r[q] + a.beta * t[q];
    }
    if (a.prev) {
        Vec<VEC>::load(a.prev + (int64_t)w.row * a.ldp + f0, t);
#pragma unroll
        for (int q = 0; q < VEC; ++q) r[q] = r[q] + a.gamma * t[q];
    }
    if (a.add) {
        Vec<VEC>::load(a.add + (int64_t)w.row * a.lda + f0, t);
#pragma unroll
        for (int q = 0; q < VEC; ++q) r[q] = r[q] + t[q];
    }
    Vec<VEC>::store(a.out + (int64_t)w.row * a.ldo + f0, r);      // after every load of this lane: out may be prev or add
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

namespace gnnmp {
namespace {

// the launch both hop exports share: `a` is complete but for rows / geom; align_extra carries the row strides' bytes into the lane-width choice
int launch_poly_hop(const char *who, const gnnmp_graph_t *plan, PolyHopArgs &a, bool scaled, uintptr_t align_extra, hipStream_t stream) {
    a.rows = plan_rows_whole(plan);
    dim3 grid;
    const int vec = row_walk_geom(who, a.rows, a.D, 0, {a.z, a.self_, a.prev, a.add, a.out}, a.geom, grid, align_extra);
    if (vec < 0) return vec;
    with_vec(vec, [&](auto V) {
        if (scaled)
            poly_hop_kernel<decltype(V)::value, 4, true><<<grid, 256, 0, stream>>>(a);
        else
            poly_hop_kernel<decltype(V)::value, 4, false><<<grid, 256, 0, stream>>>(a);
    });
    GNNMP_LAUNCH_CHECK("poly_hop_kernel");
    return GNNMP_OK;
}

// do the blocks p (rows_p rows of D floats, row stride ldp) and q share an element?  Equal strides: two column blocks of one panel are
// disjoint when their column ranges are; different strides: whether the two spans meet at all (conservative).
bool blocks_overlap(const float *p, int64_t ldp, int64_t rows_p, const float *q, int64_t ldq, int64_t rows_q, int64_t D) {
    if (!p || !q || rows_p < 1 || rows_q < 1) return false;
    const intptr_t pb = (intptr_t)reinterpret_cast<uintptr_t>(p), qb = (intptr_t)reinterpret_cast<uintptr_t>(q);
    const intptr_t pe = pb + (intptr_t)(((rows_p - 1) * ldp + D) * 4), qe = qb + (intptr_t)(((rows_q - 1) * ldq + D) * 4);
    if (pe <= qb || qe <= pb) return false;
    if (ldp != ldq) return true;
    const intptr_t ldb = (intptr_t)ldp * 4, Db = (intptr_t)D * 4;
    const intptr_t r = (((qb - pb) % ldb) + ldb) % ldb;      // q's column offset from p's inside a row, in bytes
    return r < Db || r > ldb - Db;
}

}  // namespace
}  // namespace gnnmp

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
    a.ldz = a.lds = a.ldp = a.lda = a.ldo = D;
    return launch_poly_hop(who, plan, a, job->w_slot || job->ss_slot, 0, (hipStream_t)stream);
}

extern "C" int gnnmp_poly_hop_ld_f32(const gnnmp_graph_t *plan, const gnnmp_poly_hop_ld_t *job, int64_t D, gnnmp_stream_t stream) {
    const char *who = "poly_hop_ld";
    if (!plan) return fail(GNNMP_EINVAL, "%s: null plan", who);
    if (!job) return fail(GNNMP_EINVAL, "%s: null job", who);
    if (!job->z) return fail(GNNMP_EINVAL, "%s: null z", who);
    if (!job->out) return fail(GNNMP_EINVAL, "%s: null out", who);
    if (D < 1 || D > (1 << 19)) return fail(GNNMP_EINVAL, "%s: bad D %lld (1 .. 2^19)", who, (long long)D);
    if (job->ld_z < D) return fail(GNNMP_EINVAL, "%s: ld_z %lld below D", who, (long long)job->ld_z);
    if (job->ld_out < D) return fail(GNNMP_EINVAL, "%s: ld_out %lld below D", who, (long long)job->ld_out);
    if (job->self && job->ld_self < D) return fail(GNNMP_EINVAL, "%s: ld_self %lld below D", who, (long long)job->ld_self);
    if (job->prev && job->ld_prev < D) return fail(GNNMP_EINVAL, "%s: ld_prev %lld below D", who, (long long)job->ld_prev);
    if (job->add && job->ld_add < D) return fail(GNNMP_EINVAL, "%s: ld_add %lld below D", who, (long long)job->ld_add);
    const int64_t ld_max = (int64_t)1 << 40;
    if (job->ld_z > ld_max || job->ld_out > ld_max || (job->self && job->ld_self > ld_max) || (job->prev && job->ld_prev > ld_max) ||
        (job->add && job->ld_add > ld_max))
        return fail(GNNMP_EINVAL, "%s: a row stride above 2^40", who);
    if (blocks_overlap(job->out, job->ld_out, plan->n_dst, job->z, job->ld_z, plan->n_src, D))
        return fail(GNNMP_EINVAL, "%s: out overlaps z (other lanes gather it)", who);
    if (blocks_overlap(job->out, job->ld_out, plan->n_dst, job->self, job->ld_self, plan->n_dst, D))
        return fail(GNNMP_EINVAL, "%s: out overlaps self", who);
    if (!(job->out == job->prev && job->ld_out == job->ld_prev) &&
        blocks_overlap(job->out, job->ld_out, plan->n_dst, job->prev, job->ld_prev, plan->n_dst, D))
        return fail(GNNMP_EINVAL, "%s: out overlaps prev without being it (same pointer, same stride)", who);
    if (!(job->out == job->add && job->ld_out == job->ld_add) &&
        blocks_overlap(job->out, job->ld_out, plan->n_dst, job->add, job->ld_add, plan->n_dst, D))
        return fail(GNNMP_EINVAL, "%s: out overlaps add without being it (same pointer, same stride)", who);
    if (job->beta != 0.0f && !job->self) return fail(GNNMP_EINVAL, "%s: beta != 0 with a null self", who);
    if (job->gamma != 0.0f && !job->prev) return fail(GNNMP_EINVAL, "%s: gamma != 0 with a null prev", who);
    if (plan->n_dst == 0) return GNNMP_OK;
    PolyHopArgs a = {};
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
    a.ldz = job->ld_z;
    a.ldo = job->ld_out;
    a.lds = job->self ? job->ld_self : D;
    a.ldp = job->prev ? job->ld_prev : D;
    a.lda = job->add ? job->ld_add : D;
    // a lane's 16- / 8-byte access at row i is aligned when the base and the stride's bytes are: fold the strides into the alignment word
    const uintptr_t strides = (uintptr_t)(a.ldz | a.ldo | a.lds | a.ldp | a.lda) * 4;
    return launch_poly_hop(who, plan, a, job->w_slot || job->ss_slot, strides, (hipStream_t)stream);
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
