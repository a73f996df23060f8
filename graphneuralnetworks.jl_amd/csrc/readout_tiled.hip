// readout_tiled.hip — the attention readouts of readout.hip on ROW TILES, for few, long segments (32 point clouds of 1024 points, a
// whole-graph readout): the launch shape is a function of N, G and D alone, seg_ptr is read on the device only.  include/gnnmp.h states
// the arithmetic and every fold order.
// The N rows are cut into tiles of R = GNNMP_READOUT_TILE_ROWS rows.  A PIECE is (tile t) ∩ (segment g), non-empty; the pieces form a
// monotone staircase in (t, g), so slot = t + g is unique and ascending and n_tiles + G slots always suffice: no piece table is built.
//   attn_tile_kernel        one workgroup a tile (grid.y: the feature tiles of a row wider than a lane group).  It finds its first segment
//                           by binary search in seg_ptr and walks the segments that meet the tile.  A piece of SHARE_ROWS rows or more is
//                           shared by all lane groups of the block, each taking a contiguous sub-range, their partials merged through LDS in
//                           lane-group order; shorter pieces are dealt whole to the lane groups, round robin.  x is read ONCE per row: the
//                           partial (m, den, u) is rescaled in registers whenever a row raises the maximum (one expf a row and logit).
//   attn_fold_kernel        one lane group a graph: the partials of its tiles in tile order -> r, stats (the layout of the whole-segment
//                           forward: either pullback consumes them)
//   attn_tile_grad_kernel   the same walk; per piece c_g = dr_g . r_g and α_n from stats, dx / dgate rows stored as they are met, the
//                           QUERY mode's partial dq_p = Σ ds_n x_n to the workspace
//   attn_fold_dq_kernel     dq_g = Σ_p dq_p in tile order
// No atomics; every order is fixed by (N, G, D, the alignment), so two calls give equal bits.
#include "readout.h"

namespace gnnmp {

constexpr int TILE_ROWS = GNNMP_READOUT_TILE_ROWS;
constexpr int SHARE_ROWS = 32;      // a piece at least this long is shared by the block's lane groups

struct TileWs {
    float *u;       // [n_tiles + G][D]: u_p of the forward, dq_p of the pullback
    float *md;      // [n_tiles + G][max(Dg, 1)][2]: (m_p, den_p)
};

// Calls f(g, beg, end, nk) for every piece of tile blockIdx.x in segment order, the same sequence in every thread of the block (so f may
// synchronise the block): [beg, end) are THIS lane group's rows of the piece.  nk > 0: the piece is shared, its first nk lane groups hold
// rows; nk = 0: the piece is whole in one lane group, [beg, end) is empty in the others.  Every row handed out lies in the tile and in
// [0, N), whatever the table says.
template <class F>
__device__ __forceinline__ void walk_pieces(const AttnPoolArgs &a, F &&f) {
    const int NG = 256 >> a.log2g, k = threadIdx.x >> a.log2g;
    const int64_t row0 = (int64_t)blockIdx.x * TILE_ROWS, row1 = min(row0 + TILE_ROWS, a.N);
    int64_t lo = 0, hi = a.Gn;      // the first segment that ends beyond row0
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (min(max(a.ptr[mid + 1], (int64_t)0), a.N) > row0) hi = mid;
        else lo = mid + 1;
    }
    int dealt = 0;
    for (int64_t g = lo; g < a.Gn; ++g) {
        int64_t beg, end;
        segment_of(a, g, beg, end);
        if (beg >= row1) break;
        const int64_t pb = max(beg, row0), pe = min(end, row1);
        if (pe <= pb) continue;
        if (pe - pb >= SHARE_ROWS) {
            const int64_t chunk = (pe - pb + NG - 1) / NG, b = min(pb + k * chunk, pe);
            f(g, b, min(b + chunk, pe), (int)((pe - pb + chunk - 1) / chunk));
        } else {
            f(g, pb, dealt++ % NG == k ? pe : pb, 0);
        }
    }
}

template <int VEC, int MODE>
__device__ __forceinline__ void put_partial(const AttnPoolArgs &a, const TileWs &ws, int64_t slot, int f0, bool active, int lig,
                                            const float *m, const float *den, const float *acc) {
    const int64_t D = a.D;
    if (active) {
        Vec<VEC>::store(ws.u + slot * D + f0, acc);
        if (MODE == ATTN_GATED) {
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                ws.md[(slot * D + f0 + v) * 2] = m[v];
                ws.md[(slot * D + f0 + v) * 2 + 1] = den[v];
            }
        }
    }
    if (MODE != ATTN_GATED && lig == 0 && blockIdx.y == 0) {
        ws.md[slot * 2] = m[0];
        ws.md[slot * 2 + 1] = den[0];
    }
}

template <int VEC, int MODE, bool ONE>
__global__ void __launch_bounds__(256) attn_tile_kernel(const AttnPoolArgs a, const TileWs ws) {
    constexpr int SV = MODE == ATTN_GATED ? VEC : 1;
    __shared__ float su[256 * VEC], sm[256 * SV], sd[256 * SV];
    const int G = 1 << a.log2g, tid = threadIdx.x;
    const int lig = tid & (G - 1), k = tid >> a.log2g;
    const int f0 = ((int)blockIdx.y * G + lig) * VEC;
    const bool active = f0 < a.D;
    walk_pieces(a, [&](int64_t g, int64_t beg, int64_t end, int nk) {
        float m[SV], den[SV], acc[VEC], qv[VEC];
#pragma unroll
        for (int v = 0; v < SV; ++v) {
            m[v] = -INFINITY;
            den[v] = 0.0f;
        }
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[v] = qv[v] = 0.0f;
        if (MODE == ATTN_QUERY && ONE && active) Vec<VEC>::load(a.q + g * (int64_t)a.D + f0, qv);
        sweep_rows<VEC, MODE, ONE, true>(a, g, beg, end, f0, active, lig, qv, [&](int64_t, const float (&s)[SV], const float (&xv)[VEC]) {
            float sc[SV], p[SV];
#pragma unroll
            for (int v = 0; v < SV; ++v) {      // the row raises the maximum: rescale what is held; else: its own weight.  ONE expf
                const bool up = s[v] > m[v];
                const float hi = fmaxf(m[v], s[v]), e = expf(fminf(m[v], s[v]) - hi);
                sc[v] = up ? e : 1.0f;
                p[v] = up ? 1.0f : e;
                den[v] = den[v] * sc[v] + p[v];
                m[v] = hi;
            }
#pragma unroll
            for (int v = 0; v < VEC; ++v) acc[v] = acc[v] * sc[SV == 1 ? 0 : v] + p[SV == 1 ? 0 : v] * xv[v];
        });
        const int64_t slot = (int64_t)blockIdx.x + g;
        if (nk == 0) {
            if (end > beg) put_partial<VEC, MODE>(a, ws, slot, f0, active, lig, m, den, acc);
            return;
        }
#pragma unroll
        for (int v = 0; v < VEC; ++v) su[tid * VEC + v] = acc[v];
#pragma unroll
        for (int v = 0; v < SV; ++v) {
            sm[tid * SV + v] = m[v];
            sd[tid * SV + v] = den[v];
        }
        __syncthreads();
        if (k == 0) {      // lane `lig` of every group holds the same features: the groups' partials in group order
#pragma unroll
            for (int v = 0; v < SV; ++v) {
                den[v] = 0.0f;
                for (int kk = 1; kk < nk; ++kk) m[v] = fmaxf(m[v], sm[((kk << a.log2g) + lig) * SV + v]);
            }
#pragma unroll
            for (int v = 0; v < VEC; ++v) acc[v] = 0.0f;
            for (int kk = 0; kk < nk; ++kk) {
                const int o = (kk << a.log2g) + lig;
                float w[SV];
#pragma unroll
                for (int v = 0; v < SV; ++v) {
                    w[v] = expf(sm[o * SV + v] - m[v]);
                    den[v] = den[v] + sd[o * SV + v] * w[v];
                }
#pragma unroll
                for (int v = 0; v < VEC; ++v) acc[v] = acc[v] + w[SV == 1 ? 0 : v] * su[o * VEC + v];
            }
            put_partial<VEC, MODE>(a, ws, slot, f0, active, lig, m, den, acc);
        }
        __syncthreads();
    });
}

// r and stats of graph g from the partials of its tiles, in tile order; no lane needs another's value
template <int VEC, bool PER_CHANNEL>
__global__ void __launch_bounds__(256) attn_fold_kernel(const AttnPoolArgs a, const TileWs ws) {
    constexpr int SV = PER_CHANNEL ? VEC : 1;
    const int G = 1 << a.log2g;
    const int lig = threadIdx.x & (G - 1);
    const int64_t g = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> a.log2g;
    if (g >= a.Gn) return;
    int64_t beg, end;
    segment_of(a, g, beg, end);
    const int64_t D = a.D, t0 = beg / TILE_ROWS, t1 = end > beg ? (end - 1) / TILE_ROWS : t0 - 1;
    for (int t = 0; t < a.tiles; ++t) {
        const int f0 = (t * G + lig) * VEC;
        if (f0 >= a.D) continue;
        float m[SV], den[SV], acc[VEC];
#pragma unroll
        for (int v = 0; v < SV; ++v) {
            m[v] = end > beg ? -INFINITY : 0.0f;
            den[v] = 0.0f;
        }
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[v] = 0.0f;
        for (int64_t tt = t0; tt <= t1; ++tt) {
#pragma unroll
            for (int v = 0; v < SV; ++v) m[v] = fmaxf(m[v], ws.md[(PER_CHANNEL ? (tt + g) * D + f0 + v : tt + g) * 2]);
        }
        for (int64_t tt = t0; tt <= t1; ++tt) {
            float w[SV], up[VEC];
#pragma unroll
            for (int v = 0; v < SV; ++v) {
                const int64_t o = (PER_CHANNEL ? (tt + g) * D + f0 + v : tt + g) * 2;
                w[v] = expf(ws.md[o] - m[v]);
                den[v] = den[v] + ws.md[o + 1] * w[v];
            }
            Vec<VEC>::load(ws.u + (tt + g) * D + f0, up);
#pragma unroll
            for (int v = 0; v < VEC; ++v) acc[v] = acc[v] + w[SV == 1 ? 0 : v] * up[v];
        }
        if (end > beg) {
#pragma unroll
            for (int v = 0; v < VEC; ++v) acc[v] = acc[v] / den[SV == 1 ? 0 : v];
        }
        Vec<VEC>::store(a.r + g * D + f0, acc);
        if (PER_CHANNEL) {
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                a.stats[(g * D + f0 + v) * 2] = m[v];
                a.stats[(g * D + f0 + v) * 2 + 1] = den[v];
            }
        } else if (f0 == 0) {
            a.stats[g * 2] = m[0];
            a.stats[g * 2 + 1] = den[0];
        }
    }
}

template <int VEC, int MODE, bool ONE>
__global__ void __launch_bounds__(256) attn_tile_grad_kernel(const AttnPoolArgs a, const TileWs ws) {
    constexpr int U = 4;
    constexpr int SV = MODE == ATTN_GATED ? VEC : 1;
    __shared__ float su[256 * VEC];
    const int G = 1 << a.log2g, tid = threadIdx.x;
    const int lig = tid & (G - 1), k = tid >> a.log2g;
    const int f0 = ((int)blockIdx.y * G + lig) * VEC;
    const bool active = f0 < a.D;
    const int64_t D = a.D;
    const bool want_dx = a.dx != nullptr, want_dq = MODE == ATTN_QUERY && a.dq != nullptr;
    const bool want_dgate = MODE != ATTN_QUERY && a.dgate != nullptr;
    const bool need_t = MODE == ATTN_QUERY || (MODE == ATTN_GATE1 && want_dgate);      // as in attn_pool_grad_kernel
    const bool has_base = want_dx && a.base != nullptr;
    walk_pieces(a, [&](int64_t g, int64_t beg, int64_t end, int nk) {
        float drv[VEC], qv[VEC], rv[VEC], mv[VEC], dv[VEC], dqa[VEC];
        float m1 = 0.0f, den1 = 1.0f, c = 0.0f;
        if (end > beg && MODE != ATTN_GATED) {      // (a lane group's rows are the same for all its lanes: the butterfly is whole)
            m1 = a.stats[g * 2];
            den1 = a.stats[g * 2 + 1];
            if (need_t) c = group_sum(lane_dot_tiles<VEC>(a.dr + g * D, a.r + g * D, a.D, a.tiles, G, lig), G);
        }
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
            drv[v] = qv[v] = rv[v] = dqa[v] = 0.0f;
            mv[v] = m1;
            dv[v] = den1;
        }
        if (end > beg && active) {
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
                    if (MODE == ATTN_GATE1 && want_dgate && blockIdx.y == 0 && lig == 0) a.dgate[n + u] = ds;
                }
            }
        }
        if (!want_dq) return;
        const int64_t slot = (int64_t)blockIdx.x + g;
        if (nk == 0) {
            if (end > beg && active) Vec<VEC>::store(ws.u + slot * D + f0, dqa);
            return;
        }
#pragma unroll
        for (int v = 0; v < VEC; ++v) su[tid * VEC + v] = dqa[v];
        __syncthreads();
        if (k == 0 && active) {
#pragma unroll
            for (int v = 0; v < VEC; ++v) dqa[v] = 0.0f;
            for (int kk = 0; kk < nk; ++kk) {
#pragma unroll
                for (int v = 0; v < VEC; ++v) dqa[v] = dqa[v] + su[((kk << a.log2g) + lig) * VEC + v];
            }
            Vec<VEC>::store(ws.u + slot * D + f0, dqa);
        }
        __syncthreads();
    });
}

template <int VEC>
__global__ void __launch_bounds__(256) attn_fold_dq_kernel(const AttnPoolArgs a, const TileWs ws) {
    const int G = 1 << a.log2g;
    const int lig = threadIdx.x & (G - 1);
    const int64_t g = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> a.log2g;
    if (g >= a.Gn) return;
    int64_t beg, end;
    segment_of(a, g, beg, end);
    const int64_t D = a.D, t0 = beg / TILE_ROWS, t1 = end > beg ? (end - 1) / TILE_ROWS : t0 - 1;
    for (int t = 0; t < a.tiles; ++t) {
        const int f0 = (t * G + lig) * VEC;
        if (f0 >= a.D) continue;
        float acc[VEC], part[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[v] = 0.0f;
        for (int64_t tt = t0; tt <= t1; ++tt) {
            Vec<VEC>::load(ws.u + (tt + g) * D + f0, part);
#pragma unroll
            for (int v = 0; v < VEC; ++v) acc[v] = acc[v] + part[v];
        }
        Vec<VEC>::store(a.dq + g * D + f0, acc);
    }
}

// the workspace of a tiled call and its grid; refuses a NULL workspace and what no grid can hold
static int tiled_setup(const char *who, float *workspace, int64_t N, int64_t G, int64_t D, TileWs &ws, int64_t &n_tiles) {
    if (!workspace) return fail(GNNMP_EINVAL, "%s: null workspace", who);
    n_tiles = (N + TILE_ROWS - 1) / TILE_ROWS;
    if (n_tiles >= INT32_MAX) return fail(GNNMP_EUNSUPPORTED, "%s: too many rows (%lld)", who, (long long)N);
    ws.u = workspace;
    ws.md = workspace + (n_tiles + G) * D;
    return GNNMP_OK;
}

}  // namespace gnnmp

using namespace gnnmp;

extern "C" int64_t gnnmp_segment_attn_tiled_workspace(int64_t N, int64_t G, int64_t D, int64_t Dg) {
    if (N < 0 || G < 0 || D < 1 || Dg < 0) return 0;
    return ((N + TILE_ROWS - 1) / TILE_ROWS + G) * (D + 2 * (Dg > 1 ? Dg : 1));
}

extern "C" int gnnmp_segment_attn_pool_tiled_f32(const gnnmp_segment_attn_tiled_t *job, int64_t N, int64_t G, int64_t D, int64_t Dg,
                                                 gnnmp_stream_t stream) {
    const char *who = "segment_attn_pool_tiled";
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
    GNNMP_TRY(attn_pool_setup(who, a, N, G, D, Dg, {job->x, job->q, job->r, job->workspace}, vec, mode, blocks));
    TileWs ws;
    int64_t n_tiles;
    GNNMP_TRY(tiled_setup(who, job->workspace, N, G, D, ws, n_tiles));
    if (G == 0 || N == 0) return GNNMP_OK;
    const dim3 grid((unsigned)n_tiles, (unsigned)a.tiles);
    with_vec(vec, [&](auto V) {
        with_attn_mode(mode, a.tiles == 1, [&](auto M, auto ONE) {
            attn_tile_kernel<decltype(V)::value, decltype(M)::value, decltype(ONE)::value><<<grid, 256, 0, (hipStream_t)stream>>>(a, ws);
        });
    });
    GNNMP_LAUNCH_CHECK("attn_tile_kernel");
    with_vec(vec, [&](auto V) {
        if (mode == ATTN_GATED) attn_fold_kernel<decltype(V)::value, true><<<blocks, 256, 0, (hipStream_t)stream>>>(a, ws);
        else attn_fold_kernel<decltype(V)::value, false><<<blocks, 256, 0, (hipStream_t)stream>>>(a, ws);
    });
    GNNMP_LAUNCH_CHECK("attn_fold_kernel");
    return GNNMP_OK;
}

extern "C" int gnnmp_segment_attn_pool_tiled_grad_f32(const gnnmp_segment_attn_tiled_grad_t *job, int64_t N, int64_t G, int64_t D,
                                                      int64_t Dg, gnnmp_stream_t stream) {
    const char *who = "segment_attn_pool_tiled_grad";
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
    GNNMP_TRY(attn_pool_setup(who, a, N, G, D, Dg, {job->x, job->q, job->r, job->dr, job->base, job->dq, job->dx, job->workspace}, vec, mode,
                              blocks));
    if (mode == ATTN_QUERY) {
        if (job->dgate) return fail(GNNMP_EINVAL, "%s: dgate in query mode", who);
        if (!job->dq && !job->dx) return fail(GNNMP_EINVAL, "%s: dq and dx are both null", who);
    } else {
        if (job->dq) return fail(GNNMP_EINVAL, "%s: dq in gate mode", who);
        if (!job->dgate && !job->dx) return fail(GNNMP_EINVAL, "%s: dgate and dx are both null", who);
    }
    if (job->base && !job->dx) return fail(GNNMP_EINVAL, "%s: base without dx", who);
    TileWs ws;
    int64_t n_tiles;
    GNNMP_TRY(tiled_setup(who, job->workspace, N, G, D, ws, n_tiles));
    if (G == 0 || N == 0) return GNNMP_OK;
    const dim3 grid((unsigned)n_tiles, (unsigned)a.tiles);
    with_vec(vec, [&](auto V) {
        with_attn_mode(mode, a.tiles == 1, [&](auto M, auto ONE) {
            attn_tile_grad_kernel<decltype(V)::value, decltype(M)::value, decltype(ONE)::value><<<grid, 256, 0, (hipStream_t)stream>>>(a, ws);
        });
    });
    GNNMP_LAUNCH_CHECK("attn_tile_grad_kernel");
    if (job->dq) {
        with_vec(vec, [&](auto V) { attn_fold_dq_kernel<decltype(V)::value><<<blocks, 256, 0, (hipStream_t)stream>>>(a, ws); });
        GNNMP_LAUNCH_CHECK("attn_fold_dq_kernel");
    }
    return GNNMP_OK;
}
