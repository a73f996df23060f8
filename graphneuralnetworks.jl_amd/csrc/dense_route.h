// dense_route.h — which kernel of the dense family a gnnmp_dense_f32 call reaches, which template instance of it and with what
// launch geometry: decided ONCE, on the host, as a value.  gnnmp_dense_f32 (dense.hip) builds a DenseShape and a DenseKnobs, calls
// dense_plan, keeps the DenseRoute in the calling thread's record (gnnmp_debug_dense_route) and hands it to the one launcher the
// route names (launch.h); the launchers and kernels decide nothing.  Plain C++17, no HIP header: tests/c_harness/dense_route_check.cpp
// compiles this file with g++ and tests/test_dense_route_cpu.py compares it with a restatement over a grid of shapes.
// The size functions below are the family's only definitions of them: msplit.h, mfma16.h and the .hip files use these.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <initializer_list>

#include "knobs.h"

namespace gnnmp {

// ---- sizes the kernels and the planner share (constexpr: host and device) ----------------------------------------------------------
constexpr size_t DENSE_LDS_BYTES = 160 * 1024;   // LDS of a CU: what a persistent block of the family may size itself for

// split-bf16 core (msplit.h): k-blocks of 16 positions of the concatenated contraction index
constexpr int split_nkb(int kcat) { return (kcat + 15) >> 4; }
// bytes of the three-plane image of a DP-column tile
constexpr size_t split_img_bytes(int kcat, int DP) { return (size_t)3 * split_nkb(kcat) * 2 * DP * 16; }
// threads of a dense_split_kernel block (VAR & 4: the 768 / 1024-thread experiment; default 512: 256 VGPRs)
constexpr int split_threads(int NCB, int VAR) { return (VAR & 4) ? (NCB >= 4 ? 768 : 1024) : 512; }

// 16x16x4 core (mfma16.h): rows of the W image a segment of K floats occupies (multiple of 4: a block never reads another segment's rows)
constexpr int t16_img_rows(int K) { return ((K / 4) + 3) & ~3; }
// threads per block the register budget allows: four waves per SIMD (<= 128 VGPRs) up to seven column blocks; with eight, the
// accumulators (32) + two row buffers (2 x 28-32) + the two-deep A-operand buffer (32) need ~140: three waves per SIMD
constexpr int t16_max_threads(int NCB) { return NCB >= 8 ? 768 : 1024; }

// dense_wreg_kernel: eight waves, 32 output columns each; rows of 32 image units padded to 33 (dense_wreg.hip: wr_unit)
constexpr int WR_WAVES = 8, WR_THREADS = 64 * WR_WAVES, WR_DP = 32 * WR_WAVES;
constexpr int WR_ROW = 33;

// ---- what the planner is asked ---------------------------------------------------------------------------------------------------------
struct DenseShape {
    int64_t N, D1, D2, Dout;   // validated by gnnmp_dense_f32: N >= 0, 0 < D1, Dout <= 2^20, 0 <= D2 <= 2^20
    bool x1_al16;              // x1 is 16-byte aligned
    bool x2_al16;              // x2 is 16-byte aligned (not looked at when D2 == 0)
    bool out_al16;             // out is 16-byte aligned
    bool out_al128;            // out is 128-byte aligned
};
struct DenseKnobs {           // the values of the knobs the family reads (knobs.h)
    int generic;               // KNOB_DENSE_GENERIC
    int split;                 // KNOB_DENSE_SPLIT
    int variant;               // KNOB_VARIANT
    int t16_waves;             // KNOB_DENSE_T16_WAVES
    int prefetch;              // KNOB_DENSE_PREFETCH
#ifdef GNNMP_EXPERIMENTS
    int t16_debug;             // KNOB_T16_DEBUG
#endif
};

// ---- the answer --------------------------------------------------------------------------------------------------------------------
enum DenseKernel { DENSE_NONE = 0, DENSE_SPLIT = 1, DENSE_WREG = 2, DENSE_T16 = 3, DENSE_NARROW = 4, DENSE_WLDS = 5, DENSE_MFMA = 6 };
// Sufficient to launch.  gnnmp_debug_dense_route (gnnmp.h) reports the first eight fields, the seven after `kernel` for
// dense_wlds_kernel only (zero for the others, as its contract says).  Fields a kernel does not use are zero.
struct DenseRoute {
    int kernel;     // DenseKernel; DENSE_NONE = nothing to launch (N == 0)
    int tw;         // wlds: column tile of the full launch: 128 | 64
    int waves;      // waves a block (wlds: 8 | 4; split 1..8 (12, 16 with the thread-count experiment); t16 1..16; wreg 8)
    int ks;         // wlds: columns of x staged per k-chunk (multiple of 4; = K rounded up when the whole tile fits)
    int tp;         // wlds: output column tiles per epilogue pass
    int rem_nt;     // wlds: NT of the remainder launch (0 = Dout is a multiple of tw)
    int prefetch;   // wlds: dense_wlds_kernel's pf_on, final: the kernel tests nothing else
    int full;       // wlds: column tiles of the full launch (its grid.y; 0 = only the remainder launch)
    // the template instance
    int ncb;        // split <NCB, K0C, K1C, VAR>, t16 <NCB, MAXB, KQ1, KQ2>
    int k0c, k1c;   // split, wreg <K0C, K1C>
    int var;        // split
    int maxb, kq1, kq2;   // t16
    int nout;       // narrow <NOUT>
    int nt_full;    // wlds: NT of the full launch (0 = none); rem_nt is the remainder launch's
    // the launch
    unsigned grid_x, grid_y;   // (wlds: grid_y = full; the remainder launch has grid.y 1)
    size_t lds_bytes;          // dynamic LDS
    // dense_wlds_kernel's DenseWArgs
    int xld;        // leading dimension of the wave-private x image (odd)
    int old_;       // leading dimension of the wave-private output image (multiple of 4)
    int region;     // floats per wave region
    int ktot_pad;   // rows of the W^T image
    int skew;       // s_sleep(127) repetitions for waves 4-7 before their first tile (0 = none)
    int token;      // 1 = serialise the k-loops of the two waves of a SIMD with an LDS token
    int dbg;        // t16, GNNMP_EXPERIMENTS builds: the phase ablation of KNOB_T16_DEBUG; else 0
};

// ---- acceptance predicates, in the order dense_plan asks them ---------------------------------------------------------------------------
inline bool dense_two(const DenseShape &s) { return s.D2 > 0; }

// what dense_wreg and dense_split share: the split-bf16 core is on, rows and outputs come in whole float4
inline bool split_core_takes(const DenseShape &s, const DenseKnobs &k) {
    if (k.generic != 0 || k.split < 0) return false;
    if ((s.D1 & 3) || (s.D2 & 3) || (s.Dout & 3) || s.Dout < 4 || s.N < 32) return false;
    return true;
}

// Instantiated for the layer widths of the reference's examples and benchmarks (64, 100, 128 per segment; one segment up to 256): the
// W planes of a wave's 32 columns take 12 VGPRs per 16 positions of the concatenated K — 96 (K = 128) to 192 (K = 256) of the 256 a
// wave has at two waves a SIMD.  K = 228 and 256 (100 + 128, 128 + 128, 256) were compiled too and spill 22-34 registers: left to
// dense_split's LDS-resident W, like every other shape.  Measured at N = 2.4 M, => 256 (tools/experiments/dense_wreg_ab.py, one box,
// microseconds, this kernel / dense_split): 100+100 1439 / 1578, 64+64 1006 / 1200, 64+100 1326 / 1626, 128+64 1514 / 1701, 200 1572 /
// 1670 — and one segment of K <= 128 the other way round (64: 699 / 679, 100: 922 / 871, 128: 988 / 969: not instantiated); at
// N = 5 000 the eight-wave blocks are too few (31 / 18): from 32 768 rows on.  Bit-identical to dense_split on every shape.
#define GNNMP_WREG_SHAPES(X)                                                                                       \
    X(100, 100) /* SAGEConv(100 => 256), GraphConv(100 => 256): BASELINE config 4 */                               \
    X(64, 64) X(64, 100) X(100, 64) X(64, 128) X(128, 64)                                                          \
    X(200, 0)   /* one segment: only where x is split twice by dense_split's two column passes AND K is large */
inline bool wreg_instance(int64_t D1, int64_t D2) {
#define GNNMP_WREG_IS(K0, K1) if (D1 == K0 && D2 == K1) return true;
    GNNMP_WREG_SHAPES(GNNMP_WREG_IS)
#undef GNNMP_WREG_IS
    return false;
}
// 256 outputs (SAGEConv(100 => 256)): W in registers, x through LDS once (dense_wreg.hip)
inline bool wreg_takes(const DenseShape &s, const DenseKnobs &k) {
    if (!split_core_takes(s, k)) return false;
    if (k.variant & VARIANT_NO_WREG) return false;       // (A/B runs)
    if (s.Dout != WR_DP || s.N < ((k.variant & VARIANT_WREG_SMALL) ? 4096 : 32768) || s.N > (int64_t)INT32_MAX - 64) return false;      // (row numbers of a tile are 32-bit)
    if (!s.x1_al16 || !s.out_al128) return false;
    if (dense_two(s) && !s.x2_al16) return false;
    return wreg_instance(s.D1, s.D2);
}

// NCB of dense_split_kernel: the widest column tile whose image fits: fewer passes over x; 0 = neither fits
inline int split_ncb(const DenseShape &s) {
    const int kcat = (int)(s.D1 + s.D2);
    const size_t budget = DENSE_LDS_BYTES - 1024;
    if (s.Dout > 64 && split_img_bytes(kcat, 128) <= budget) return 4;
    if (split_img_bytes(kcat, 64) <= budget) return 2;
    return 0;
}
// round 3: the split-bf16 core (three exact bf16 planes per operand, six bf16 MFMAs per product: fp32-class accuracy at
// 2.7x the fp32-MFMA rate) for every shape whose W image fits LDS
inline bool split_takes(const DenseShape &s, const DenseKnobs &k) {
    if (!split_core_takes(s, k)) return false;
    // column blocks are 32 wide: a Dout that pads by more than a tenth (100 -> 128) costs more MFMA work and a select per stored piece
    // than the fp32 16x16x4 kernel's 16-wide blocks (measured 2.4 M x 100 => 100: 625 us here, 549 us there)
    if (((s.Dout + 31) & ~(int64_t)31) * 10 > s.Dout * 11) return false;
    if (!s.x1_al16 || !s.out_al16) return false;
    if (dense_two(s) && !s.x2_al16) return false;
    return split_ncb(s) != 0;
}

// the shapes of the hot path (K a multiple of 4, <= 128 per segment): operands straight from HBM, 16x16x4 MFMAs
inline bool t16_takes(const DenseShape &s, const DenseKnobs &k) {
    if (k.generic != 0) return false;
    if ((s.D1 & 3) || (s.D2 & 3) || s.D1 > 128 || s.D2 > 128 || (s.Dout & 3) || s.Dout < 4) return false;
    if (!s.x1_al16 || !s.out_al16) return false;
    if (dense_two(s) && !s.x2_al16) return false;
    if (s.N < 16) return false;
    return true;
}

// Dout <= 8 (a classifier head): eight lanes per row, no matrix core (dense.hip: dense_narrow_kernel)
inline bool narrow_takes(const DenseShape &s, const DenseKnobs &k) {
    if (k.generic != 0) return false;
    if (s.Dout > 8 || (s.D1 & 3) || (s.D2 & 3) || s.D1 > 4096 || s.D2 > 4096) return false;
    if (!s.x1_al16 || (s.D2 > 0 && !s.x2_al16)) return false;
    return true;
}

// dense_wlds_kernel's LDS sizing for a column tile of tw columns; waves == 0: W^T plus the wave regions do not fit
struct WldsCfg { int tw, waves, ks, xld, old_, tp; size_t wbytes, region; };
constexpr size_t WLDS_BUDGET = DENSE_LDS_BYTES - 64;   // 4 pipe tokens live after the wave regions
inline WldsCfg wlds_size_for(const DenseShape &s, int tw) {
    const int64_t Dout = s.Dout;
    const int k0p = ((int)s.D1 + 1) & ~1, k1p = ((int)s.D2 + 1) & ~1;
    const int ktot = k0p + (s.D2 > 0 ? k1p : 0);
    const int kmax = std::max(k0p, k1p);
    const size_t budget = WLDS_BUDGET;
    WldsCfg c{};
    c.tw = tw;
    const int full = (int)(Dout / tw), rem = (int)(Dout % tw);
    const int nt_max = full > 0 ? tw / 32 : (rem + 31) / 32;
    const int ncols_max = full > 0 ? tw : rem;
    c.wbytes = (size_t)ktot * (size_t)(nt_max * 32 + 1) * sizeof(float);
    // Wave regions: prefer 8 waves per CU.  If the whole 32 x K image does not leave room for 8 regions, stage x
    // in k-chunks (ks columns at a time); only if even 48-column chunks do not fit, fall back to 4 waves.
    for (int wv : {8, 4}) {  // fewer than one wave per SIMD cannot feed the matrix pipe: K-chunked kernel instead
        if (c.wbytes >= budget) break;
        const int cols_fit = (int)((budget - c.wbytes) / ((size_t)wv * 32 * sizeof(float)));  // floats per region row
        int kfit = ((cols_fit - 1) & ~3);               // leave the +1 (odd leading dimension)
        kfit = std::min(kfit, (kmax + 3) & ~3);
        kfit = std::min(kfit, 128);                      // <= 32 float4 per staged row (shift-mapped staging)
        if (kfit >= ((kmax + 3) & ~3) || kfit >= 48) {   // (24-column chunks measured slower than 4 waves x 44)
            const int nkc = (kmax + kfit - 1) / kfit;     // balanced chunks, multiple of 4
            c.ks = (((kmax + nkc - 1) / nkc) + 3) & ~3;
            c.waves = wv;
            break;
        }
    }
    c.xld = c.ks + 1;                                   // odd: conflict-free A-operand reads
    // the wave region is sized for the x image (>= one 32-column output tile); the output tile passes through it
    // whole if it fits, else tp column tiles at a time
    const int region_cols = (std::max(c.xld, 32) + 3) & ~3;
    c.tp = 4;
    c.old_ = (ncols_max + 3) & ~3;
    if (c.old_ > region_cols) {
        c.tp = region_cols / 32;
        c.old_ = c.tp * 32;
    }
    c.region = (size_t)32 * (size_t)region_cols;
    if (c.waves > 0 && c.wbytes + (size_t)c.waves * c.region * sizeof(float) > budget) c.waves = 0;
    return c;
}
// W-resident kernel when W^T (for one column tile) plus the wave regions fit the 160 KB LDS.  The column tile is 128
// wide unless that leaves room for only 4 waves (K1 + K2 around 256): then 64-wide tiles — x is staged twice, but 8
// waves (two per SIMD) overlap one wave's staging with the other's MFMAs (GraphConv 128 => 128: see LABNOTES.md).
inline WldsCfg wlds_cfg(const DenseShape &s) {
    WldsCfg c = wlds_size_for(s, 128);
    if (c.waves < 8 && s.Dout >= 128) {
        const WldsCfg c64 = wlds_size_for(s, 64);
        if (c64.waves == 8) c = c64;
    }
    return c;
}
inline bool wlds_takes(const DenseShape &s, const DenseKnobs &k, const WldsCfg &c) {
    return c.waves > 0 && s.N >= 256 && k.generic != 1;
}

// ---- per kernel: the instance and the launch geometry of a shape it takes -----------------------------------------------------------
inline void plan_wreg(DenseRoute &r, const DenseShape &s, int cus) {
    r.kernel = DENSE_WREG;
    r.k0c = (int)s.D1; r.k1c = (int)s.D2;
    const int NKB = split_nkb(r.k0c + r.k1c);
    r.lds_bytes = (size_t)2 * 3 * NKB * 2 * WR_ROW * 16 + (size_t)WR_DP * 4 + (size_t)WR_WAVES * 4096;
    const int64_t ntiles = (s.N + 31) / 32;
    r.waves = WR_WAVES;
    r.grid_x = (unsigned)std::min<int64_t>(cus, ntiles);
    r.grid_y = 1;
}

inline void plan_split(DenseRoute &r, const DenseShape &s, const DenseKnobs &k, int cus) {
    r.kernel = DENSE_SPLIT;
    const bool two = dense_two(s);
    const int kcat = (int)(s.D1 + s.D2), nkb = split_nkb(kcat);
    const int NCB = split_ncb(s), DP = NCB * 32;
    // K known at compile time for the shapes of the configs (K0C = 0: any K; K1C = 1 then stands for "two segments")
    r.ncb = NCB;
    r.k0c = 0; r.k1c = two ? 1 : 0;
    auto known = [&](int K0C, int K1C) { if (s.D1 == K0C && s.D2 == K1C) { r.k0c = K0C; r.k1c = K1C; } };
    if (NCB == 4) {
        known(16, 16);      // GraphConv 16 + 16 => 128
        known(100, 100);    // SAGEConv 100 + 100 => 256 (two column tiles)
        known(100, 0);      // 100 => 100 | 128 (GCNConv, GATConv dense_x: products)
        known(128, 0);      // 128 => 128 (arxiv)
    } else {
        known(128, 128);    // GraphConv 128 + 128 => 128 (two column tiles)
    }
    // stores through the per-wave LDS stage (whole 128-byte lines) when 8 stages fit beside the image (VARIANT_SPLIT_DIRECT_STORES = never, for A/B runs)
    const bool staged = split_img_bytes(nkb * 16, NCB * 32) + (size_t)NCB * 32 * 4 + 8 * 4096 <= DENSE_LDS_BYTES && !(k.variant & VARIANT_SPLIT_DIRECT_STORES);
    int VAR = (s.Dout % (NCB * 32) == 0 ? 256 : 0) | (staged ? 4096 : 0);
#ifdef GNNMP_EXPERIMENTS
    if ((r.k0c == 100 && r.k1c == 0) || (r.k0c == 128 && r.k1c == 128)) {   // knob 13 selects a variant, on two shapes only (build time)
        for (int v : {257, 258, 260, 1280, 2304, 264, 272, 320, 384, 400, 768})
            if (k.t16_debug == v) VAR = v;
    }
#endif
    r.var = VAR;
    r.lds_bytes = split_img_bytes(nkb * 16, DP) + (size_t)DP * 4 + ((VAR & 4096) ? (size_t)(split_threads(NCB, VAR) / 64) * 4096 : 0);
    const int64_t ntiles = (s.N + 31) / 32;
    const int max_waves = split_threads(NCB, VAR) / 64;
    int waves = (int)std::min<int64_t>(max_waves, std::max<int64_t>(4, (ntiles + cus - 1) / cus));
    if (ntiles < (int64_t)cus * max_waves * 8) {
        // few tiles per wave (arxiv shape: 5 292 tiles, 2.6 per wave at 8 waves a block): the last round of the wave-major hand-out is
        // partly empty — pick the wave count whose rounds are fullest (arxiv: 7 waves -> 2.95 tiles per wave, 98 % instead of 86 %)
        double best = -1.0;
        for (int w = max_waves; w >= 4; --w) {
            const int64_t slots = (int64_t)cus * w;
            const double eff = (double)ntiles / (double)(((ntiles + slots - 1) / slots) * slots);
            if (eff > best + 0.02) { best = eff; waves = w; }
        }
    }
    const int kw = k.t16_waves;
    if (kw >= 1 && kw <= max_waves) waves = kw;
    r.waves = waves;
    // Several column tiles (Dout > DP: SAGEConv's 256 columns are two): a block fills a CU (LDS), so with `cus` blocks per column tile
    // the tiles ran one after the other and x came from HBM once per column tile.  cus / ny blocks per column tile instead: blocks
    // (b, 0), (b, 1), ... walk the same row tiles at the same time and — linear block ids b, b + gx, ... with gx a multiple of 8 — on
    // the same XCD, so every read of x after the first is an L2 hit (VARIANT_SPLIT_SERIAL_TILES = the old grid, for A/B runs).
    const int ny = (int)((s.Dout + DP - 1) / DP);
    int64_t bx = cus;
    if (ny > 1 && !(k.variant & VARIANT_SPLIT_SERIAL_TILES)) bx = std::max<int64_t>(8, (int64_t)(cus / ny) & ~(int64_t)7);
    const int64_t gx = std::min<int64_t>(bx, (ntiles + waves - 1) / waves);
    r.grid_x = (unsigned)gx;
    r.grid_y = (unsigned)ny;
}

inline void plan_t16(DenseRoute &r, const DenseShape &s, const DenseKnobs &k, int cus) {
    r.kernel = DENSE_T16;
    // column blocks of 16 per column tile: as few padded columns as the shape allows (100 -> 7 x 16 = 112, not 128)
    const int cb = (int)((s.Dout + 15) / 16);
    const int kq1 = (int)s.D1 / 4, kq2 = (int)s.D2 / 4;
    r.maxb = 8; r.kq1 = -1; r.kq2 = -1;       // any K
    auto known = [&](int MAXB, int KQ1, int KQ2) { if (kq1 == KQ1 && kq2 == KQ2) { r.maxb = MAXB; r.kq1 = KQ1; r.kq2 = KQ2; } };
    if (cb > 8 || cb == 8) {
        // 128-column tiles (grid.y of them): the shapes of the configs first, K known at compile time
        r.ncb = 8;
        known(7, 25, 0);      // GATConv dense_x 100 => 128
        known(8, 32, 0);      // arxiv 128 => 128
        known(7, 25, 25);     // SAGEConv 100 + 100 => 256
        known(8, 32, 32);     // GraphConv 128 + 128 => 128
        known(1, 4, 4);       // GraphConv 16 + 16 => 128
    } else if (cb == 7) {
        r.ncb = 7;
        known(7, 25, 0);      // GCNConv 100 => 100
    } else if (cb > 4) {
        r.ncb = 6;
    } else if (cb > 2) {
        r.ncb = 4;
    } else {
        r.ncb = 2;
    }
    const int DP = r.ncb * 16;
    const int rows = t16_img_rows((int)s.D1) + (dense_two(s) ? t16_img_rows((int)s.D2) : 0);
    r.lds_bytes = (size_t)rows * DP * 16 + (size_t)DP * 4;
    const int64_t ntiles = (s.N + 15) / 16;
    // waves per block: 16 (four per SIMD) on large inputs; on small ones fewer, so that every CU gets a block
    const int max_waves = t16_max_threads(r.ncb) / 64;
    int waves = (int)std::min<int64_t>(max_waves, std::max<int64_t>(4, (ntiles + cus - 1) / cus));
    const int kw = k.t16_waves;
    if (kw >= 1 && kw <= max_waves) waves = kw;
    r.waves = waves;
#ifdef GNNMP_EXPERIMENTS
    r.dbg = k.t16_debug;
#endif
    const int64_t gx = std::min<int64_t>(cus, (ntiles + waves - 1) / waves);
    r.grid_x = (unsigned)gx;
    r.grid_y = (unsigned)((s.Dout + DP - 1) / DP);
}

inline void plan_narrow(DenseRoute &r, const DenseShape &s) {
    r.kernel = DENSE_NARROW;
    r.nout = s.Dout <= 2 ? 2 : (s.Dout <= 4 ? 4 : 8);
    r.grid_x = (unsigned)((s.N * 8 + 255) / 256);
    r.grid_y = 1;
}

inline void plan_wlds(DenseRoute &r, const DenseShape &s, const DenseKnobs &k, const WldsCfg &c, int cus) {
    r.kernel = DENSE_WLDS;
    const int k0p = ((int)s.D1 + 1) & ~1, k1p = ((int)s.D2 + 1) & ~1;
    const int ktot = k0p + (s.D2 > 0 ? k1p : 0);
    r.tw = c.tw;
    r.waves = c.waves;
    r.xld = c.xld;
    r.old_ = c.old_;
    r.tp = c.tp;
    r.ks = c.ks;
    r.skew = k.prefetch & 15;          // experiment knob (slot 7): low 4 bits = s_sleep(127) count,
    r.token = (k.prefetch >> 4) & 1;   //                           bit 4 = matrix-pipe token
    const int pf_knob = ((k.prefetch >> 5) & 1) ^ 1;   //           bit 5 = cross-tile prefetch OFF
    // Cross-tile prefetch: one segment, whole-K staging, 16-byte-aligned rows (K a multiple of 4 and x1 aligned).  This is the
    // kernel's pf_on: dense_wlds_kernel takes the value as it is.
    r.prefetch = pf_knob && !dense_two(s) && r.ks >= (((int)s.D1 + 1) & ~1) && (s.D1 & 3) == 0 && s.x1_al16;
    r.region = (int)c.region;
    r.ktot_pad = ktot;
    const int64_t n_row_tiles = (s.N + 31) / 32;
    r.lds_bytes = c.wbytes + (size_t)c.waves * c.region * sizeof(float) + 16;   // + 4 pipe tokens
    const int full = (int)(s.Dout / c.tw), rem = (int)(s.Dout % c.tw);
    r.full = full;
    r.nt_full = full > 0 ? c.tw / 32 : 0;
    r.rem_nt = (rem + 31) / 32;
    int64_t gx = (n_row_tiles + r.waves - 1) / r.waves;
    if (gx > cus) gx = cus;  // one persistent block per CU (the LDS image allows no more)
    r.grid_x = (unsigned)gx;
    r.grid_y = (unsigned)full;
}

// dense_mfma_kernel's block tile (dense.hip): 128 x 128, k-chunks of 32
constexpr int MFMA_BM = 128, MFMA_BN = 128;
inline void plan_mfma(DenseRoute &r, const DenseShape &s) {
    r.kernel = DENSE_MFMA;
    r.grid_x = (unsigned)((s.N + MFMA_BM - 1) / MFMA_BM);
    r.grid_y = (unsigned)((s.Dout + MFMA_BN - 1) / MFMA_BN);
}

// ---- the planner: top to bottom is the priority order ------------------------------------------------------------------------------
inline DenseRoute dense_plan(const DenseShape &s, const DenseKnobs &k, int cus) {
    DenseRoute r{};
    if (s.N == 0) return r;
    if (wreg_takes(s, k)) { plan_wreg(r, s, cus); return r; }
    if (split_takes(s, k)) { plan_split(r, s, k, cus); return r; }
    if (t16_takes(s, k)) { plan_t16(r, s, k, cus); return r; }
    if (narrow_takes(s, k)) { plan_narrow(r, s); return r; }
    const WldsCfg c = wlds_cfg(s);
    if (wlds_takes(s, k, c)) { plan_wlds(r, s, k, c, cus); return r; }
    plan_mfma(r, s);   // the K-chunked kernel takes everything
    return r;
}

}  // namespace gnnmp
