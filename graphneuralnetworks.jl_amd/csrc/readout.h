// readout.h — what the attention readout kernels of readout.hip (one lane group a segment) and readout_tiled.hip (row tiles) share:
// the argument record, the lane-group folds, the row sweep, the refusals and the geometry of a call.
#pragma once
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
