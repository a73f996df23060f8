// readout.hip — the graph-level readouts with attention, forward and pullback, as segment kernels: Set2Set's per-iteration
// softmax-weighted sum (set2set_pool, GNNlib/src/layers/pool.jl:29-43) and GlobalAttentionPool (pool.jl:7-12), plus the pullback of
// Flux.LSTMCell's pointwise part.  include/gnnmp.h states the arithmetic.
//   attn_pool_kernel       one lane group finishes one graph (segment_pool_ptr_kernel's geometry, leaf.hip): lanes run over features,
//                          U = 4 rows in flight.  THREE sweeps over the segment: max of the logits, den = Σ exp(s - m), then
//                          r = Σ α_n x_n with α_n = exp(s_n - m) / den — the second and third sweep find the rows in L1 / L2.  QUERY mode:
//                          the logit s_n = q_g . x_n is each lane's partial over its features (ascending) folded across the group by an
//                          xor butterfly; GATE mode: the logits are read, one per row (Dg = 1) or one per channel (Dg = D).
//   attn_pool_grad_kernel  ONE sweep: c_g = dr_g . r_g first, then per row α_n recomputed from stats, t_n = dr_g . x_n folded like the
//                          logit, ds_n = α_n (t_n - c_g); dq_g accumulates in registers, dx / dgate rows are stored as they are met
//   lstm_pointwise_grad_kernel   elementwise, the gates recomputed from gx + gh + b by lstm_pointwise_kernel's expressions
// A row wider than one group's lanes is covered by FEATURE TILES walked by the same lane group, one after the other (the logit needs the
// whole row, so the tiles cannot go to different groups): with more than one tile the logit loop reads the whole row once per tile —
// correct for any D up to GNNMP_READOUT_MAX_D, quadratic in the tile count, meant for the occasional wide or odd D.
// No atomics, no scratch, every output element written exactly once (empty segments included: zeros), two calls give equal bits.
// A SEGMENT OF ANY LENGTH IS WALKED BY ITS ONE LANE GROUP: correct, slow for whole-graph readouts of millions of rows.
#include "common.h"

namespace gnnmp {

enum { ATTN_QUERY = 0, ATTN_GATE1 = 1, ATTN_GATED = 2 };

struct AttnPoolArgs {
    const float *x;          // [N][D]
    const int64_t *ptr;      // [Gn + 1]
    const float *q;          // [Gn][D], QUERY
    const float *gate;       // [N][Dg], GATE1 / GATED
    float *r;                // [Gn][D]; the pullback reads it
    float *stats;            // [Gn][max(Dg, 1)][2]; the pullback reads it
    // the pullback only
    const float *dr;         // [Gn][D]
    const float *base;       // [N][D] or null; may be dx
    float *dq;               // [Gn][D] or null
    float *dx;               // [N][D] or null
    float *dgate;            // [N][Dg] or null
    int D, log2g, tiles;
    int64_t N, Gn;
};

// sum over the G lanes (a power of two <= 64) of a lane group; every lane of the group is active (they share the trip counts)
__device__ __forceinline__ float group_sum(float v, int G) {
    for (int o = G >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// this lane's share of a . b over ALL feature tiles, features ascending (two rows of D floats)
template <int VEC>
__device__ __forceinline__ float lane_dot_tiles(const float *a, const float *b, int D, int tiles, int G, int lig) {
    float part = 0.0f;
    for (int t = 0; t < tiles; ++t) {
        const int f = (t * G + lig) * VEC;
        if (f < D) {
            float av[VEC], bv[VEC];
            Vec<VEC>::load(a + f, av);
            Vec<VEC>::load(b + f, bv);
#pragma unroll
            for (int v = 0; v < VEC; ++v) part = part + av[v] * bv[v];
        }
    }
    return part;
}

// the segment of graph g, clamped into [0, N]: a bad table cannot send a lane out of x
__device__ __forceinline__ void segment_of(const AttnPoolArgs &a, int64_t g, int64_t &beg, int64_t &end) {
    beg = min(max(a.ptr[g], (int64_t)0), a.N);
    end = min(max(a.ptr[g + 1], beg), a.N);
}

// Calls f(u-th row's logits s[SV], its x vector at this lane's features) for every row of [beg, end) in node order, U rows in flight.
// QUERY / GATE1: SV = 1 and s is uniform over the group; GATED: SV = VEC, one logit per channel.  ONE: the row fits one feature tile
// (QUERY: the vector loaded for the logit is the one handed on).  NEED_X: f reads the x vector.
template <int VEC, int MODE, bool ONE, bool NEED_X, class F>
__device__ __forceinline__ void sweep_rows(const AttnPoolArgs &a, int64_t g, int64_t beg, int64_t end, int f0, bool active, int lig,
                                           const float (&qv)[VEC], F &&f) {
    constexpr int U = 4;
    constexpr int SV = MODE == ATTN_GATED ? VEC : 1;
    const int G = 1 << a.log2g;
    const int64_t D = a.D;
    for (int64_t n = beg; n < end; n += U) {
        float xv[U][VEC], s[U][SV];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t nn = min(n + u, end - 1);      // clamped, unconditional within the lane's activity
#pragma unroll
            for (int v = 0; v < VEC; ++v) xv[u][v] = 0.0f;
#pragma unroll
            for (int v = 0; v < SV; ++v) s[u][v] = 0.0f;
            if ((NEED_X || (MODE == ATTN_QUERY && ONE)) && active) Vec<VEC>::load(a.x + nn * D + f0, xv[u]);
            if (MODE == ATTN_QUERY) {
                if (ONE) {
#pragma unroll
                    for (int v = 0; v < VEC; ++v) s[u][0] = s[u][0] + qv[v] * xv[u][v];
                } else {
                    s[u][0] = lane_dot_tiles<VEC>(a.q + g * D, a.x + nn * D, a.D, a.tiles, G, lig);
                }
            } else if (MODE == ATTN_GATE1) {
                s[u][0] = a.gate[nn];
            } else if (active) {
                Vec<VEC>::load(a.gate + nn * D + f0, s[u]);
            }
        }
        if (MODE == ATTN_QUERY) {
#pragma unroll
            for (int u = 0; u < U; ++u) s[u][0] = group_sum(s[u][0], G);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (n + u < end) f(n + u, s[u], xv[u]);
        }
    }
}

template <int VEC, int MODE, bool ONE>
__global__ void __launch_bounds__(256) attn_pool_kernel(const AttnPoolArgs a) {
    constexpr int SV = MODE == ATTN_GATED ? VEC : 1;
    const int G = 1 << a.log2g;
    const int lig = threadIdx.x & (G - 1);
    const int64_t g = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> a.log2g;
    if (g >= a.Gn) return;
    int64_t beg, end;
    segment_of(a, g, beg, end);
    const int64_t D = a.D;
    float m[SV], den[SV];
    for (int t = 0; t < a.tiles; ++t) {
        const int f0 = (t * G + lig) * VEC;
        const bool active = f0 < a.D;
        float qv[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) qv[v] = 0.0f;
        if (MODE == ATTN_QUERY && ONE && active) Vec<VEC>::load(a.q + g * D + f0, qv);
        if (MODE == ATTN_GATED || t == 0) {      // QUERY / GATE1: one (m, den) per graph, found once
#pragma unroll
            for (int v = 0; v < SV; ++v) m[v] = -INFINITY;
            sweep_rows<VEC, MODE, ONE, false>(a, g, beg, end, f0, active, lig, qv, [&](int64_t, const float (&s)[SV], const float (&)[VEC]) {
#pragma unroll
                for (int v = 0; v < SV; ++v) m[v] = fmaxf(m[v], s[v]);
            });
#pragma unroll
            for (int v = 0; v < SV; ++v) {
                if (end == beg) m[v] = 0.0f;
                den[v] = 0.0f;
            }
            sweep_rows<VEC, MODE, ONE, false>(a, g, beg, end, f0, active, lig, qv, [&](int64_t, const float (&s)[SV], const float (&)[VEC]) {
#pragma unroll
                for (int v = 0; v < SV; ++v) den[v] = den[v] + expf(s[v] - m[v]);
            });
        }
        float acc[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[v] = 0.0f;
        sweep_rows<VEC, MODE, ONE, true>(a, g, beg, end, f0, active, lig, qv, [&](int64_t, const float (&s)[SV], const float (&xv)[VEC]) {
            float al[SV];
#pragma unroll
            for (int v = 0; v < SV; ++v) al[v] = expf(s[v] - m[v]) / den[v];
#pragma unroll
            for (int v = 0; v < VEC; ++v) acc[v] = acc[v] + al[SV == 1 ? 0 : v] * xv[v];
        });
        if (active) {
            Vec<VEC>::store(a.r + g * D + f0, acc);
            if (MODE == ATTN_GATED) {
#pragma unroll
                for (int v = 0; v < VEC; ++v) {
                    a.stats[(g * D + f0 + v) * 2] = m[SV == 1 ? 0 : v];
                    a.stats[(g * D + f0 + v) * 2 + 1] = den[SV == 1 ? 0 : v];
                }
            }
        }
    }
    if (MODE != ATTN_GATED && lig == 0) {
        a.stats[g * 2] = m[0];
        a.stats[g * 2 + 1] = den[0];
    }
}

template <int VEC, int MODE, bool ONE>
__global__ void __launch_bounds__(256) attn_pool_grad_kernel(const AttnPoolArgs a) {
    constexpr int U = 4;
    constexpr int SV = MODE == ATTN_GATED ? VEC : 1;
    const int G = 1 << a.log2g;
    const int lig = threadIdx.x & (G - 1);
    const int64_t g = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> a.log2g;
    if (g >= a.Gn) return;
    int64_t beg, end;
    segment_of(a, g, beg, end);
    const int64_t D = a.D;
    const bool want_dx = a.dx != nullptr, want_dq = MODE == ATTN_QUERY && a.dq != nullptr;
    const bool want_dgate = MODE != ATTN_QUERY && a.dgate != nullptr;
    // ds_n = α_n (dr . x_n - c) is wanted by everything in QUERY mode and by dgate alone under GATE1
    const bool need_t = MODE == ATTN_QUERY || (MODE == ATTN_GATE1 && want_dgate);
    float m1 = 0.0f, den1 = 1.0f, c = 0.0f;
    if (MODE != ATTN_GATED) {
        m1 = a.stats[g * 2];
        den1 = a.stats[g * 2 + 1];
        if (need_t) c = group_sum(lane_dot_tiles<VEC>(a.dr + g * D, a.r + g * D, a.D, a.tiles, G, lig), G);
    }
    for (int t = 0; t < a.tiles; ++t) {
        const int f0 = (t * G + lig) * VEC;
        const bool active = f0 < a.D;
        float drv[VEC], qv[VEC], rv[VEC], mv[VEC], dv[VEC], dqa[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
            drv[v] = qv[v] = rv[v] = dqa[v] = 0.0f;
            mv[v] = m1;
            dv[v] = den1;
        }
        if (active) {
            Vec<VEC>::load(a.dr + g * D + f0, drv);
            if (MODE == ATTN_QUERY) Vec<VEC>::load(a.q + g * D + f0, qv);
            if (MODE == ATTN_GATED) {
                Vec<VEC>::load(a.r + g * D + f0, rv);
#pragma unroll
                for (int v = 0; v < VEC; ++v) {
                    mv[v] = a.stats[(g * D + f0 + v) * 2];
                    dv[v] = a.stats[(g * D + f0 + v) * 2 + 1];
                }
            }
        }
        for (int64_t n = beg; n < end; n += U) {
            float xv[U][VEC], bv[U][VEC], s[U][SV], tt[U];
            const bool has_base = want_dx && a.base != nullptr;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t nn = min(n + u, end - 1);
#pragma unroll
                for (int v = 0; v < VEC; ++v) xv[u][v] = bv[u][v] = 0.0f;
#pragma unroll
                for (int v = 0; v < SV; ++v) s[u][v] = 0.0f;
                tt[u] = 0.0f;
                if (active) {
                    Vec<VEC>::load(a.x + nn * D + f0, xv[u]);
                    if (has_base) Vec<VEC>::load(a.base + nn * D + f0, bv[u]);
                }
                if (MODE == ATTN_QUERY) {
                    if (ONE) {
#pragma unroll
                        for (int v = 0; v < VEC; ++v) s[u][0] = s[u][0] + qv[v] * xv[u][v];
                    } else {
                        s[u][0] = lane_dot_tiles<VEC>(a.q + g * D, a.x + nn * D, a.D, a.tiles, G, lig);
                    }
                } else if (MODE == ATTN_GATE1) {
                    s[u][0] = a.gate[nn];
                } else if (active) {
                    Vec<VEC>::load(a.gate + nn * D + f0, s[u]);
                }
                if (need_t) {
                    if (ONE) {
#pragma unroll
                        for (int v = 0; v < VEC; ++v) tt[u] = tt[u] + drv[v] * xv[u][v];
                    } else {
                        tt[u] = lane_dot_tiles<VEC>(a.dr + g * D, a.x + nn * D, a.D, a.tiles, G, lig);
                    }
                }
            }
            if (MODE == ATTN_QUERY) {
#pragma unroll
                for (int u = 0; u < U; ++u) s[u][0] = group_sum(s[u][0], G);
            }
            if (need_t) {
#pragma unroll
                for (int u = 0; u < U; ++u) tt[u] = group_sum(tt[u], G);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (n + u < end) {
                    float al[VEC], o[VEC], dg[VEC] = {};
#pragma unroll
                    for (int v = 0; v < VEC; ++v) al[v] = expf(s[u][SV == 1 ? 0 : v] - mv[v]) / dv[v];
                    const float ds = al[0] * (tt[u] - c);      // QUERY / GATE1 (al is uniform there)
#pragma unroll
                    for (int v = 0; v < VEC; ++v) {
                        o[v] = al[v] * drv[v];
                        if (MODE == ATTN_GATED) dg[v] = o[v] * (xv[u][v] - rv[v]);
                        if (has_base) o[v] = bv[u][v] + o[v];
                        if (MODE == ATTN_QUERY) {
                            o[v] = o[v] + ds * qv[v];
                            dqa[v] = dqa[v] + ds * xv[u][v];
                        }
                    }
                    if (active) {
                        if (want_dx) Vec<VEC>::store(a.dx + (n + u) * D + f0, o);
                        if (MODE == ATTN_GATED && want_dgate) Vec<VEC>::store(a.dgate + (n + u) * D + f0, dg);
                    }
                    if (MODE == ATTN_GATE1 && want_dgate && t == 0 && lig == 0) a.dgate[n + u] = ds;
                }
            }
        }
        if (want_dq && active) Vec<VEC>::store(a.dq + g * D + f0, dqa);
    }
}

// pullback of lstm_pointwise_kernel (leaf.hip): the gates by the same expressions, then the chain rule term by term
__global__ void __launch_bounds__(256) lstm_pointwise_grad_kernel(const float *__restrict__ gx, const float *__restrict__ gh,
                                                                  const float *__restrict__ b, const float *__restrict__ c,
                                                                  const float *__restrict__ dh, const float *__restrict__ dcn,
                                                                  float *__restrict__ da, float *__restrict__ dc, int64_t N, int D) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N * D) return;
    const int64_t n = i / D;
    const int d = (int)(i - n * D);
    const int64_t o = n * 4 * D + d;
    float g4[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) g4[q] = gx[o + q * D] + gh[o + q * D] + (b ? b[q * D + d] : 0.0f);
    auto sg = [](float x) { const float t = expf(-fabsf(x)); return x >= 0.0f ? 1.0f / (1.0f + t) : t / (1.0f + t); };
    const float gi = sg(g4[0]), gf = sg(g4[1]), gc = tanhf(g4[2]), go = sg(g4[3]);
    const float cv = c[i];
    const float tc = tanhf(gf * cv + gi * gc);
    const float dhv = dh[i];
    const float dct = (dcn ? dcn[i] : 0.0f) + dhv * go * (1.0f - tc * tc);
    da[o] = dct * gc * (gi * (1.0f - gi));
    da[o + D] = dct * cv * (gf * (1.0f - gf));
    da[o + 2 * (int64_t)D] = dct * gi * (1.0f - gc * gc);
    da[o + 3 * (int64_t)D] = dhv * tc * (go * (1.0f - go));
    dc[i] = dct * gf;
}

// what both segment exports refuse, and their geometry; the vector width is the one every array of the call admits
static int attn_pool_setup(const char *who, AttnPoolArgs &a, int64_t N, int64_t G, int64_t D, int64_t Dg,
                           std::initializer_list<const float *> ptrs, int &vec, int &mode, unsigned &blocks) {
    if (N < 0 || G < 0) return fail(GNNMP_EINVAL, "%s: negative N %lld or G %lld", who, (long long)N, (long long)G);
    if (D < 1 || D > GNNMP_READOUT_MAX_D)
        return fail(GNNMP_EINVAL, "%s: bad D %lld (1 .. %d)", who, (long long)D, GNNMP_READOUT_MAX_D);
    if (Dg != 0 && Dg != 1 && Dg != D) return fail(GNNMP_EINVAL, "%s: bad Dg %lld (0, 1 or D = %lld)", who, (long long)Dg, (long long)D);
    if ((a.q != nullptr) == (a.gate != nullptr)) return fail(GNNMP_EINVAL, "%s: exactly one of q and gate must be given", who);
    if ((a.q != nullptr) != (Dg == 0)) return fail(GNNMP_EINVAL, "%s: Dg %lld does not go with %s", who, (long long)Dg, a.q ? "q" : "gate");
    mode = Dg == 0 ? ATTN_QUERY : Dg == 1 ? ATTN_GATE1 : ATTN_GATED;      // (D = 1: the one-channel gate)
    uintptr_t align = 0;
    for (const float *p : ptrs) align |= reinterpret_cast<uintptr_t>(p);
    if (mode == ATTN_GATED) align |= reinterpret_cast<uintptr_t>(a.gate) | reinterpret_cast<uintptr_t>(a.dgate);
    vec = pick_vec(D, reinterpret_cast<const void *>(align), nullptr);
    a.log2g = pick_log2g((D + vec - 1) / vec);
    a.tiles = feature_tiles(D, vec, a.log2g);
    a.D = (int)D;
    a.N = N;
    a.Gn = G;
    const int64_t nb = ((G << a.log2g) + 255) / 256;
    if (nb >= INT32_MAX) return fail(GNNMP_EUNSUPPORTED, "%s: too many graphs (%lld)", who, (long long)G);
    blocks = (unsigned)nb;
    return GNNMP_OK;
}

template <class F>
static void with_attn_mode(int mode, bool one, F &&f) {
    if (mode == ATTN_QUERY) return one ? f(int_c<ATTN_QUERY>{}, std::true_type{}) : f(int_c<ATTN_QUERY>{}, std::false_type{});
    if (mode == ATTN_GATE1) return one ? f(int_c<ATTN_GATE1>{}, std::true_type{}) : f(int_c<ATTN_GATE1>{}, std::false_type{});
    return f(int_c<ATTN_GATED>{}, std::false_type{});      // per channel: nothing crosses the tiles
}

}  // namespace gnnmp

using namespace gnnmp;

extern "C" int gnnmp_segment_attn_pool_f32(const gnnmp_segment_attn_t *job, int64_t N, int64_t G, int64_t D, int64_t Dg,
                                           gnnmp_stream_t stream) {
    const char *who = "segment_attn_pool";
    if (!job) return fail(GNNMP_EINVAL, "%s: null job", who);
    if (!job->x && N > 0) return fail(GNNMP_EINVAL, "%s: null x", who);
    if (!job->seg_ptr) return fail(GNNMP_EINVAL, "%s: null seg_ptr", who);
    if (!job->r) return fail(GNNMP_EINVAL, "%s: null r", who);
    if (!job->stats) return fail(GNNMP_EINVAL, "%s: null stats", who);
    AttnPoolArgs a = {};
    a.x = job->x;
    a.ptr = job->seg_ptr;
    a.q = job->q;
    a.gate = job->gate;
    a.r = job->r;
    a.stats = job->stats;
    int vec, mode;
    unsigned blocks;
    GNNMP_TRY(attn_pool_setup(who, a, N, G, D, Dg, {job->x, job->q, job->r}, vec, mode, blocks));
    if (G == 0 || N == 0) return GNNMP_OK;
    with_vec(vec, [&](auto V) {
        with_attn_mode(mode, a.tiles == 1, [&](auto M, auto ONE) {
            attn_pool_kernel<decltype(V)::value, decltype(M)::value, decltype(ONE)::value><<<blocks, 256, 0, (hipStream_t)stream>>>(a);
        });
    });
    GNNMP_LAUNCH_CHECK("attn_pool_kernel");
    return GNNMP_OK;
}

extern "C" int gnnmp_segment_attn_pool_grad_f32(const gnnmp_segment_attn_grad_t *job, int64_t N, int64_t G, int64_t D, int64_t Dg,
                                                gnnmp_stream_t stream) {
    const char *who = "segment_attn_pool_grad";
    if (!job) return fail(GNNMP_EINVAL, "%s: null job", who);
    if (!job->x && N > 0) return fail(GNNMP_EINVAL, "%s: null x", who);
    if (!job->seg_ptr) return fail(GNNMP_EINVAL, "%s: null seg_ptr", who);
    if (!job->dr) return fail(GNNMP_EINVAL, "%s: null dr", who);
    if (!job->r) return fail(GNNMP_EINVAL, "%s: null r", who);
    if (!job->stats) return fail(GNNMP_EINVAL, "%s: null stats", who);
    AttnPoolArgs a = {};
    a.x = job->x;
    a.ptr = job->seg_ptr;
    a.q = job->q;
    a.gate = job->gate;
    a.r = const_cast<float *>(job->r);          // read only by the pullback
    a.stats = const_cast<float *>(job->stats);
    a.dr = job->dr;
    a.base = job->base;
    a.dq = job->dq;
    a.dx = job->dx;
    a.dgate = job->dgate;
    int vec, mode;
    unsigned blocks;
    GNNMP_TRY(attn_pool_setup(who, a, N, G, D, Dg, {job->x, job->q, job->r, job->dr, job->base, job->dq, job->dx}, vec, mode, blocks));
    if (mode == ATTN_QUERY) {
        if (job->dgate) return fail(GNNMP_EINVAL, "%s: dgate in query mode", who);
        if (!job->dq && !job->dx) return fail(GNNMP_EINVAL, "%s: dq and dx are both null", who);
    } else {
        if (job->dq) return fail(GNNMP_EINVAL, "%s: dq in gate mode", who);
        if (!job->dgate && !job->dx) return fail(GNNMP_EINVAL, "%s: dgate and dx are both null", who);
    }
    if (job->base && !job->dx) return fail(GNNMP_EINVAL, "%s: base without dx", who);
    if (G == 0 || N == 0) return GNNMP_OK;
    with_vec(vec, [&](auto V) {
        with_attn_mode(mode, a.tiles == 1, [&](auto M, auto ONE) {
            attn_pool_grad_kernel<decltype(V)::value, decltype(M)::value, decltype(ONE)::value><<<blocks, 256, 0, (hipStream_t)stream>>>(a);
        });
    });
    GNNMP_LAUNCH_CHECK("attn_pool_grad_kernel");
    return GNNMP_OK;
}

extern "C" int gnnmp_lstm_pointwise_grad_f32(const gnnmp_lstm_grad_t *job, int64_t N, int64_t D, gnnmp_stream_t stream) {
    const char *who = "lstm_pointwise_grad";
    if (!job) return fail(GNNMP_EINVAL, "%s: null job", who);
    if (N < 0) return fail(GNNMP_EINVAL, "%s: negative N %lld", who, (long long)N);
    if (D < 1 || D > (1 << 20)) return fail(GNNMP_EINVAL, "%s: bad D %lld (1 .. 2^20)", who, (long long)D);
    if (!job->gx || !job->gh || !job->c || !job->dh) return fail(GNNMP_EINVAL, "%s: null gx, gh, c or dh", who);
    if (!job->da || !job->dc) return fail(GNNMP_EINVAL, "%s: null da or dc", who);
    if (N == 0) return GNNMP_OK;
    if ((N * D + 255) / 256 >= INT32_MAX) return fail(GNNMP_EUNSUPPORTED, "%s: N * D too large", who);
    lstm_pointwise_grad_kernel<<<(unsigned)((N * D + 255) / 256), 256, 0, (hipStream_t)stream>>>(job->gx, job->gh, job->b, job->c, job->dh,
                                                                                                  job->dcn, job->da, job->dc, N, (int)D);
    GNNMP_LAUNCH_CHECK("lstm_pointwise_grad_kernel");
    return GNNMP_OK;
}
