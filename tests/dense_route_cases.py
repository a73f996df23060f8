"""The grid of gnnmp_dense_f32 calls that pins the dense family's routing, shared by tests/test_dense_route_cpu.py (the planner of
csrc/dense_route.h under plain g++), tests/test_dense_routes.py (the library's hook on the GPU) and the script that recorded
tests/golden/dense_routes_v1.json; and `restated`, the route written out by hand from the five host paths the planner replaced
(gnnmp_dense_f32, dense_split_try with launch_split and launch_split_var, dense_wreg_try, dense_t16_try with launch_t16,
dense_narrow_try), each in its own words."""
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "dense_routes_v1.json")

NONE, SPLIT, WREG, T16, NARROW, WLDS, MFMA = range(7)         # DenseKernel (csrc/dense_route.h) = info[0] of the hook
GENERIC, PREFETCH, T16_WAVES, DENSE_SPLIT, VARIANT = 6, 7, 12, 17, 19          # knob numbers (csrc/knobs.h)
SERIAL_TILES, DIRECT_STORES, NO_WREG, WREG_SMALL = 16, 32, 64, 512             # bits of knob 19

# ---- the grid ---------------------------------------------------------------------------------------------------------------------
DOUTS = [2, 4, 8, 10, 47, 64, 65, 100, 111, 112, 128, 130, 200, 256]
# segment widths crossed with every Dout: the compile-time widths of the hot kernels (100, 128, 16 + 16, 100 + 100, 128 + 128), a
# dense_wreg pair, an odd K, multiples of 4 above dense_t16's 128, and 512: 32 k-blocks, neither split image (128 or 64 columns) fits
KPAIRS = [(100, 0), (128, 0), (64, 0), (7, 0), (132, 0), (200, 0), (16, 16), (100, 100), (128, 128), (64, 100), (512, 0)]
# tests/test_dense_fallbacks.py: TABLE and MFMA_ONLY (copied: that module is marked gpu as a whole)
FALLBACK_TABLE = {
    (100, 0, 111): dict(tw=128, waves=8, chunks=1, tp=3, nt=4, pf=1),
    (100, 0, 47): dict(tw=128, waves=8, chunks=1, tp=4, nt=2, pf=1),
    (64, 0, 10): dict(tw=128, waves=8, chunks=1, tp=4, nt=1, pf=1),
    (7, 0, 47): dict(tw=128, waves=8, chunks=1, tp=1, nt=2, pf=0),
    (3, 0, 130): dict(tw=128, waves=8, chunks=1, tp=1, nt=1, pf=0),
    (36, 0, 65): dict(tw=128, waves=8, chunks=1, tp=1, nt=3, pf=1),
    (129, 0, 100): dict(tw=128, waves=8, chunks=2, tp=2, nt=4, pf=0),
    (200, 0, 100): dict(tw=128, waves=8, chunks=4, tp=1, nt=4, pf=0),
    (256, 0, 47): dict(tw=128, waves=8, chunks=3, tp=4, nt=2, pf=0),
    (257, 0, 100): dict(tw=128, waves=4, chunks=5, tp=1, nt=4, pf=0),
    (300, 0, 70): dict(tw=128, waves=4, chunks=4, tp=4, nt=3, pf=0),
    (127, 127, 130): dict(tw=64, waves=8, chunks=2, tp=4, nt=1, pf=0),
    (150, 150, 200): dict(tw=64, waves=8, chunks=2, tp=4, nt=1, pf=0),
    (130, 126, 128): dict(tw=64, waves=8, chunks=2, tp=4, nt=0, pf=0),
    (100, 100, 47): dict(tw=128, waves=8, chunks=1, tp=4, nt=2, pf=0),
    (16, 100, 47): dict(tw=128, waves=8, chunks=1, tp=4, nt=2, pf=0),
}
MFMA_ONLY = [(1433, 0, 130), (700, 700, 16)]
WREG_PAIRS = [(100, 100), (64, 64), (64, 100), (100, 64), (64, 128), (128, 64), (200, 0)]      # dense_wreg's instances, Dout 256
# Dout <= 8: segment widths at, below and above dense_narrow's 4096, in either segment
NARROW_SHAPES = [(K1, K2, D) for (K1, K2) in ((4096, 0), (4100, 0), (8, 4096), (4, 4100), (4092, 4096)) for D in (2, 4, 8)]


# five and six column blocks of 16: dense_t16's NCB = 6 instance (no Dout of the list above lies in 68..96)
T16_SIX = [(100, 0, 80), (64, 64, 96)]


def _shapes():
    out = []
    for s in ([(K1, K2, D) for (K1, K2) in KPAIRS for D in DOUTS] + list(FALLBACK_TABLE) + MFMA_ONLY +
              [(K1, K2, 256) for (K1, K2) in WREG_PAIRS] + NARROW_SHAPES + T16_SIX):
        if s not in out:
            out.append(s)
    return out


SHAPES = _shapes()
NS = [0, 15, 16, 31, 32, 255, 256, 4095, 4096, 32767, 32768]
CUS = [8, 256, 304]
KNOBS = [                                                     # (name, {knob: value}); 17 is knob 7's default
    ("default", {}),
    ("generic1", {GENERIC: 1}),
    ("generic2", {GENERIC: 2}),
    ("nosplit", {DENSE_SPLIT: -1}),
    ("no_wreg", {VARIANT: NO_WREG}),
    ("wreg_small", {VARIANT: WREG_SMALL}),
    ("serial_tiles", {VARIANT: SERIAL_TILES}),
    ("direct_stores", {VARIANT: DIRECT_STORES}),
    ("t16_waves3", {T16_WAVES: 3}),
    ("prefetch17", {PREFETCH: 17}),
    ("prefetch49", {PREFETCH: 49}),
    ("prefetch0", {PREFETCH: 0}),
]
# The four alignment facts of DenseShape are x1, x2, out 16-byte aligned and out 128-byte aligned.  The GPU recording states them with real
# buffers: (x1, x2, out) offsets in floats into a 256-byte-aligned allocation — 1 float
# leaves 4-byte alignment, 4 floats 16-byte but not 128-byte alignment
OFFSETS = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 4), (1, 1, 1)]


def facts_of(off):
    x1o, x2o, oo = off
    return (int(x1o % 4 == 0), int(x2o % 4 == 0), int(oo % 4 == 0), int(oo % 32 == 0))


def gpu_ns(shape):
    """the recording's rows: N <= 4096 and x no larger than 4096 x 1433 (the 4096-wide segments stop at 256 rows), and the dense_wreg
    threshold for the 256-column shapes"""
    return [n for n in NS if (n <= 4096 and n * max(shape[:2]) <= 4096 * 1433) or shape[2] == 256]


def gpu_offsets(shape):
    return [o for o in OFFSETS if shape[1] > 0 or o[1] == 0 or o == (1, 1, 1)]


# ---- the recording ----------------------------------------------------------------------------------------------------------------
# {"commit", "what", "cus", "knobs", "info": the distinct eight-int vectors, "lists": the distinct lists, over gpu_ns(shape) x
# gpu_offsets(shape), of indices into "info", "rows": {"K1,K2,Dout": [per knob setting, an index into "lists"]}}
def load_golden():
    with open(GOLDEN) as f:
        g = json.load(f)
    assert g["knobs"] == [[n, {str(k): v for k, v in kv.items()}] for n, kv in KNOBS], "the recording was made for another knob list"
    rows = []
    for shape in SHAPES:
        per_knob = g["rows"]["%d,%d,%d" % shape]
        assert len(per_knob) == len(KNOBS)
        for (name, kv), li in zip(KNOBS, per_knob):
            idx = g["lists"][li]
            cells = [(n, o) for n in gpu_ns(shape) for o in gpu_offsets(shape)]
            assert len(idx) == len(cells)
            for (n, o), i in zip(cells, idx):
                rows.append((shape, n, o, kv, g["info"][i]))
    return g, rows


# ---- the restatement --------------------------------------------------------------------------------------------------------------
FIELDS = ("kernel", "tw", "waves", "ks", "tp", "rem_nt", "prefetch", "full", "ncb", "k0c", "k1c", "var", "maxb", "kq1", "kq2", "nout",
          "nt_full", "grid_x", "grid_y", "lds_bytes", "xld", "old", "region", "ktot_pad", "skew", "token")
LDS = 160 * 1024


def _ceil(a, b):
    return -(-a // b)


def _route(**kw):
    r = dict.fromkeys(FIELDS, 0)
    r.update(kw)
    return r


def _split_or_wreg(K1, K2, Dout, N, x1a, x2a, o16, o128, cus, kn):
    """dense_split_try, with dense_wreg_try called from its middle"""
    two = K2 > 0
    variant = kn.get(VARIANT, 0)
    if kn.get(GENERIC, 0) != 0 or kn.get(DENSE_SPLIT, 0) < 0:
        return None
    if K1 % 4 or K2 % 4 or Dout % 4 or Dout < 4 or N < 32:
        return None
    ntiles = _ceil(N, 32)
    # dense_wreg_try
    if not variant & NO_WREG and Dout == 256 and N >= (4096 if variant & WREG_SMALL else 32768) and N <= 2 ** 31 - 1 - 64 \
            and x1a and o128 and (x2a or not two) and (K1, K2) in WREG_PAIRS:
        nkb = _ceil(K1 + K2, 16)
        return _route(kernel=WREG, k0c=K1, k1c=K2, waves=8, grid_x=min(cus, ntiles), grid_y=1,
                      lds_bytes=2 * 3 * nkb * 2 * 33 * 16 + 256 * 4 + 8 * 4096)
    if _ceil(Dout, 32) * 32 * 10 > Dout * 11:
        return None
    if not x1a or not o16 or (two and not x2a):
        return None
    kcat = K1 + K2
    nkb = _ceil(kcat, 16)

    def img(dp):
        return 3 * nkb * 2 * dp * 16

    budget = LDS - 1024
    if Dout > 64 and img(128) <= budget:
        ncb = 4
        if two:
            inst = (K1, K2) if (K1, K2) in ((16, 16), (100, 100)) else (0, 1)
        else:
            inst = (K1, 0) if K1 in (100, 128) else (0, 0)
    elif img(64) <= budget:
        ncb = 2
        if two:
            inst = (128, 128) if (K1, K2) == (128, 128) else (0, 1)
        else:
            inst = (0, 0)
    else:
        return None
    dp = ncb * 32
    # launch_split (release build: no experiment variants)
    staged = img(dp) + dp * 4 + 8 * 4096 <= LDS and not variant & DIRECT_STORES
    var = (256 if Dout % dp == 0 else 0) | (4096 if staged else 0)
    # launch_split_var: 512 threads
    max_waves = 8
    lds = img(dp) + dp * 4 + (max_waves * 4096 if staged else 0)
    waves = min(max_waves, max(4, _ceil(ntiles, cus)))
    if ntiles < cus * max_waves * 8:
        best = -1.0
        for w in range(max_waves, 3, -1):
            slots = cus * w
            eff = ntiles / (_ceil(ntiles, slots) * slots)
            if eff > best + 0.02:
                best, waves = eff, w
    kw = kn.get(T16_WAVES, 0)
    if 1 <= kw <= max_waves:
        waves = kw
    ny = _ceil(Dout, dp)
    bx = cus
    if ny > 1 and not variant & SERIAL_TILES:
        bx = max(8, (cus // ny) & ~7)
    return _route(kernel=SPLIT, ncb=ncb, k0c=inst[0], k1c=inst[1], var=var, waves=waves, grid_x=min(bx, _ceil(ntiles, waves)),
                  grid_y=ny, lds_bytes=lds)


def _t16(K1, K2, Dout, N, x1a, x2a, o16, o128, cus, kn):
    """dense_t16_try and launch_t16"""
    if kn.get(GENERIC, 0) != 0:
        return None
    if K1 % 4 or K2 % 4 or K1 > 128 or K2 > 128 or Dout % 4 or Dout < 4:
        return None
    if not x1a or not o16 or (K2 > 0 and not x2a) or N < 16:
        return None
    cb = _ceil(Dout, 16)
    kq = (K1 // 4, K2 // 4)
    rt = (8, -1, -1)
    if cb >= 8:
        ncb = 8
        inst = {(25, 0): (7, 25, 0), (32, 0): (8, 32, 0), (25, 25): (7, 25, 25), (32, 32): (8, 32, 32), (4, 4): (1, 4, 4)}.get(kq, rt)
    elif cb == 7:
        ncb = 7
        inst = (7, 25, 0) if kq == (25, 0) else rt
    else:
        ncb = 6 if cb > 4 else (4 if cb > 2 else 2)
        inst = rt
    dp = ncb * 16

    def rows(K):
        return (K // 4 + 3) // 4 * 4

    lds = (rows(K1) + (rows(K2) if K2 > 0 else 0)) * dp * 16 + dp * 4
    ntiles = _ceil(N, 16)
    max_waves = 12 if ncb >= 8 else 16
    waves = min(max_waves, max(4, _ceil(ntiles, cus)))
    kw = kn.get(T16_WAVES, 0)
    if 1 <= kw <= max_waves:
        waves = kw
    return _route(kernel=T16, ncb=ncb, maxb=inst[0], kq1=inst[1], kq2=inst[2], waves=waves, grid_x=min(cus, _ceil(ntiles, waves)),
                  grid_y=_ceil(Dout, dp), lds_bytes=lds)


def _narrow(K1, K2, Dout, N, x1a, x2a, o16, o128, cus, kn):
    """dense_narrow_try, which gnnmp_dense_f32 calls only with knob 6 at 0"""
    if kn.get(GENERIC, 0) != 0:
        return None
    if Dout > 8 or K1 % 4 or K2 % 4 or K1 > 4096 or K2 > 4096 or not x1a or (K2 > 0 and not x2a):
        return None
    return _route(kernel=NARROW, nout=2 if Dout <= 2 else (4 if Dout <= 4 else 8), grid_x=_ceil(N * 8, 256), grid_y=1)


def _wlds_size_for(tw, K1, K2, Dout):
    k0p, k1p = (K1 + 1) // 2 * 2, (K2 + 1) // 2 * 2
    ktot = k0p + (k1p if K2 > 0 else 0)
    kmax = max(k0p, k1p)
    budget = LDS - 64
    full, rem = divmod(Dout, tw)
    nt_max = tw // 32 if full else _ceil(rem, 32)
    ncols_max = tw if full else rem
    wbytes = ktot * (nt_max * 32 + 1) * 4
    waves = ks = 0
    kneed = _ceil(kmax, 4) * 4
    for wv in (8, 4):
        if wbytes >= budget:
            break
        cols_fit = (budget - wbytes) // (wv * 32 * 4)
        kfit = min((cols_fit - 1) // 4 * 4, kneed, 128)
        if kfit >= kneed or kfit >= 48:
            nkc = _ceil(kmax, kfit)
            ks = _ceil(_ceil(kmax, nkc), 4) * 4
            waves = wv
            break
    xld = ks + 1
    region_cols = _ceil(max(xld, 32), 4) * 4
    tp, old = 4, _ceil(ncols_max, 4) * 4
    if old > region_cols:
        tp = region_cols // 32
        old = tp * 32
    region = 32 * region_cols
    if waves > 0 and wbytes + waves * region * 4 > budget:
        waves = 0
    return dict(tw=tw, waves=waves, ks=ks, xld=xld, old=old, tp=tp, wbytes=wbytes, region=region, ktot=ktot)


def _wlds(K1, K2, Dout, N, x1a, x2a, o16, o128, cus, kn):
    """the W-resident branch of gnnmp_dense_f32"""
    c = _wlds_size_for(128, K1, K2, Dout)
    if c["waves"] < 8 and Dout >= 128:
        c64 = _wlds_size_for(64, K1, K2, Dout)
        if c64["waves"] == 8:
            c = c64
    if not (c["waves"] > 0 and N >= 256 and kn.get(GENERIC, 0) != 1):
        return None
    k7 = kn.get(PREFETCH, 17)
    full, rem = divmod(Dout, c["tw"])
    pf = (not (k7 >> 5) & 1) and K2 == 0 and c["ks"] >= (K1 + 1) // 2 * 2 and K1 % 4 == 0 and x1a
    return _route(kernel=WLDS, tw=c["tw"], waves=c["waves"], ks=c["ks"], tp=c["tp"], rem_nt=_ceil(rem, 32), prefetch=int(bool(pf)),
                  full=full, nt_full=(c["tw"] // 32 if full else 0), grid_x=min(cus, _ceil(_ceil(N, 32), c["waves"])), grid_y=full,
                  lds_bytes=c["wbytes"] + c["waves"] * c["region"] * 4 + 16, xld=c["xld"], old=c["old"], region=c["region"],
                  ktot_pad=c["ktot"], skew=k7 & 15, token=(k7 >> 4) & 1)


def restated(shape, N, facts, cus, kn):
    """the route of one call as a dict over FIELDS: the parent's order split (with wreg inside) -> t16 -> narrow -> wlds -> mfma"""
    K1, K2, Dout = shape
    if N == 0:
        return _route()
    args = (K1, K2, Dout, N) + tuple(facts) + (cus, kn)
    for path in (_split_or_wreg, _t16, _narrow, _wlds):
        r = path(*args)
        if r is not None:
            return r
    return _route(kernel=MFMA, grid_x=_ceil(N, 128), grid_y=_ceil(Dout, 128))
