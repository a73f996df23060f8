"""The three fp32 fallbacks of gnnmp_dense_f32 (csrc/dense.hip) at the shapes that reach them with DEFAULT knobs: dense_wlds_kernel
(W resident in LDS; odd K or Dout, a misaligned operand, K > 128 onto a width that pads badly), dense_mfma_kernel (K-chunked: N < 256,
or a W image that does not fit LDS) and dense_narrow_kernel (Dout <= 8).  The hot kernels (dense_split, dense_t16) refuse these shapes.

Every call goes through the C ABI with `out` carved out of a larger buffer (32 sentinel rows on either side), and every call asserts
the ROUTE it was written for: gnnmp_debug_dense_route reports the kernel and, for dense_wlds_kernel, the host-chosen configuration
(column tile, waves, k-chunk, epilogue passes, NT of the remainder launch, whether the cross-tile prefetch condition held).

Two element-wise checks per case:
  exact   operands are integers in -3..3 and the bias in -8..8: every product and partial sum is an integer below 2^24, exact in fp32
          in ANY summation order (and in three bf16 planes), so the output must EQUAL the integer product.  The reference is the float64
          product, which holds these integers exactly as well (|sum| < 2^53).  A dropped, doubled or misplaced k-term, a wrong tail
          column or a stale LDS row cannot hide behind a tolerance.
  gauss   Gaussian operands against float64: |y - ref| <= (K1 + K2 + 2) * 2^-24 * (sum_k |w_k x_k| + |b|) per element, the standard
          bound of K products and K + 1 additions in fp32 in any order (derived, not measured).

Rows: 255 (the dispatcher's threshold: dense_mfma_kernel) and 256 (dense_wlds_kernel), 256 + 32 + 5 (a ragged last tile), and
32 * CUs * waves * 2 + 32 * 3 + 7 on a subset: there some waves of the persistent blocks take two row tiles, some three, and the last
tile is ragged, so the cross-tile prefetch hands over full -> full and full -> ragged."""
import ctypes

import pytest

pytestmark = pytest.mark.gpu

NONE, SPLIT, WREG, T16, NARROW, WLDS, MFMA = range(7)         # info[0] of gnnmp_debug_dense_route (include/gnnmp.h)
SENTINEL = -3.0e38                                           # no result of these tests comes near it
GUARD_ROWS = 32
U = 2.0 ** -24

# (K1, K2, Dout): tw, waves, k-chunks of the longer segment, tp, NT of the remainder launch, prefetch condition — what
# wlds_size_for (csrc/dense_route.h) gives for the shape; the hook is the authority, every wlds call asserts these against it, and
# tests/test_dense_route_cpu.py asks the planner itself for these sixteen
TABLE = {
    (100, 0, 111): dict(tw=128, waves=8, chunks=1, tp=3, nt=4, pf=1),       # whole-K staging, two epilogue passes of 96 + 15 columns
    (100, 0, 47): dict(tw=128, waves=8, chunks=1, tp=4, nt=2, pf=1),        # a classifier head
    (64, 0, 10): dict(tw=128, waves=8, chunks=1, tp=4, nt=1, pf=1),
    (7, 0, 47): dict(tw=128, waves=8, chunks=1, tp=1, nt=2, pf=0),          # odd K: the zeroed second column of the last k-step
    (3, 0, 130): dict(tw=128, waves=8, chunks=1, tp=1, nt=1, pf=0),         # one full 128 tile (NT 4, four passes) + a 2-column remainder
    (36, 0, 65): dict(tw=128, waves=8, chunks=1, tp=1, nt=3, pf=1),
    (129, 0, 100): dict(tw=128, waves=8, chunks=2, tp=2, nt=4, pf=0),       # odd K in two chunks
    (200, 0, 100): dict(tw=128, waves=8, chunks=4, tp=1, nt=4, pf=0),
    (256, 0, 47): dict(tw=128, waves=8, chunks=3, tp=4, nt=2, pf=0),
    (257, 0, 100): dict(tw=128, waves=4, chunks=5, tp=1, nt=4, pf=0),       # four waves: no SIMD partner, no token
    (300, 0, 70): dict(tw=128, waves=4, chunks=4, tp=4, nt=3, pf=0),
    (127, 127, 130): dict(tw=64, waves=8, chunks=2, tp=4, nt=1, pf=0),      # 64-wide tiles: two full + remainder
    (150, 150, 200): dict(tw=64, waves=8, chunks=2, tp=4, nt=1, pf=0),      # three full + remainder
    (130, 126, 128): dict(tw=64, waves=8, chunks=2, tp=4, nt=0, pf=0),      # no remainder; the chunk width comes from segment 1
    (100, 100, 47): dict(tw=128, waves=8, chunks=1, tp=4, nt=2, pf=0),      # two segments, whole-K
    (16, 100, 47): dict(tw=128, waves=8, chunks=1, tp=4, nt=2, pf=0),       # the chunk width comes from segment 2
}
SHAPES = list(TABLE)
PREFETCH_SHAPES = [s for s in SHAPES if TABLE[s]["pf"]]
# the derived row count: the three prefetch-on shapes of the classifier-head kind, one chunked, one 4-wave and one 64-wide-tile shape
LARGE_SHAPES = [(100, 0, 111), (100, 0, 47), (64, 0, 10), (200, 0, 100), (257, 0, 100), (127, 127, 130)]
MFMA_ONLY = [(1433, 0, 130), (700, 700, 16)]                  # the W image does not fit LDS: K-chunked at default knobs too
# (layout, padded ldw, bias, relu): a half fraction of the 2^4 design — every factor half on, every pair of factors fully crossed
VARIANTS = [(l, (l + b + a) & 1, b, a) for l in (0, 1) for b in (0, 1) for a in (0, 1)]
SMALL_ROWS = (255, 256, 256 + 32 + 5)

RECORDS = []      # (K1, K2, Dout, N, info[8]) of every dense_wlds_kernel route seen by this module


def ident(s):
    return "K%d+%d_D%d" % s


@pytest.fixture(scope="module")
def gm():
    import torch
    assert torch.cuda.is_available()
    import gnnmp
    gnnmp.load()
    return gnnmp


def route():
    from gnnmp import _lib as L
    info = (ctypes.c_int * 8)()
    L.check(L.load().gnnmp_debug_dense_route(info))
    return list(info)


def chunks_of(K1, K2, ks):
    return -(-max((K1 + 1) & ~1, (K2 + 1) & ~1) // ks)


class Case:
    """operands of one product and its float64 reference; computed once, called as often as a test likes"""

    def __init__(self, shape, N, kind, w_layout=0, pad=0, bias=1, act=0, x_off=0, seed=0):
        import torch
        K1, K2, Dout = shape
        self.shape, self.N, self.act, self.w_layout = shape, N, act, w_layout
        g = torch.Generator(device="cuda")
        g.manual_seed(1 + seed + 1000 * (K1 + 7 * K2 + 13 * Dout) + N)

        def draw(size, lim, sd):
            if kind == "exact":
                return torch.randint(-lim, lim + 1, size, device="cuda", generator=g).float()
            return torch.randn(size, device="cuda", generator=g) * sd

        def place_x(v):           # x_off = 1: a view one float into its buffer (4-byte aligned only)
            buf = torch.empty(v.numel() + 4, device="cuda")
            buf[x_off:x_off + v.numel()] = v.flatten()
            return buf[x_off:x_off + v.numel()].view(v.shape)

        def place_w(w):           # w [Dout][K] -> the layout's matrix inside rows of ldw floats; the padding is NaN and never read
            m = w if w_layout == 0 else w.t()
            ldw = m.shape[1] + (3 if pad else 0)
            buf = torch.full((m.shape[0], ldw), float("nan"), device="cuda")
            buf[:, :m.shape[1]] = m
            return buf, ldw

        self.xs = [place_x(draw((N, K), 3, 1.0)) for K in (K1, K2) if K]
        ws = [draw((Dout, K), 3, 0.3) for K in (K1, K2) if K]
        self.Ws = [place_w(w) for w in ws]
        self.b = draw((Dout,), 8, 0.2) if bias else None
        assert self.xs[0].data_ptr() % 16 == 4 * x_off
        self.ws64 = [w.double() for w in ws]
        self.reference()

    def reference(self):
        import torch
        pre = sum(x.double() @ w.t() for x, w in zip(self.xs, self.ws64))
        mag = sum(x.double().abs() @ w.abs().t() for x, w in zip(self.xs, self.ws64))
        if self.b is not None:
            pre, mag = pre + self.b.double(), mag + self.b.double().abs()
        self.ref = torch.relu(pre) if self.act else pre
        self.mag = mag

    def run(self, out_off=0):
        """-> (out, info): out a view into a buffer with GUARD_ROWS sentinel rows before and after (checked here)"""
        import torch
        from gnnmp import _lib as L
        K1, K2, Dout = self.shape
        N, g = self.N, GUARD_ROWS * Dout
        buf = torch.full(((N + 2 * GUARD_ROWS) * Dout + 4,), SENTINEL, device="cuda")
        out = buf[g + out_off:g + out_off + N * Dout].view(N, Dout)
        assert out.data_ptr() % 16 == 4 * out_off
        x2, (W2, ldw2) = (self.xs[1], self.Ws[1]) if K2 else (None, (None, 0))
        L.check(L.load().gnnmp_dense_f32(L.ptr(self.xs[0]), L.ptr(self.Ws[0][0]), K1, self.Ws[0][1], L.ptr(x2), L.ptr(W2), K2, ldw2,
                                         self.w_layout, L.ptr(self.b), self.act, L.ptr(out), N, Dout, L.stream_ptr()))
        info = route()
        assert bool((buf[:g + out_off] == SENTINEL).all()) and bool((buf[g + out_off + N * Dout:] == SENTINEL).all()), \
            f"{self}: a guard row was written"
        if info[0] == WLDS:
            RECORDS.append((K1, K2, Dout, N, info))
        return out, info

    def __str__(self):
        return "K=%d+%d Dout=%d N=%d layout=%d act=%d" % (*self.shape, self.N, self.w_layout, self.act)


def check(case, kind, y, tag):
    """the module's two checks, element-wise; the message carries the count and place of the wrong elements / the worst error"""
    K1, K2, _ = case.shape
    if kind == "exact":
        wrong = (y.double() != case.ref).nonzero()
        assert wrong.numel() == 0, f"{case} {tag}: {wrong.shape[0]} elements differ from the integer product, first at {wrong[0].tolist()}"
    else:
        bound = (K1 + K2 + 2) * U
        worst = float(((y.double() - case.ref).abs() / case.mag).max())
        assert worst <= bound, f"{case} {tag}: error {worst:.3e} of sum|w||x| + |b| exceeds (K + 2) * 2^-24 = {bound:.3e}"


def expect_wlds(case, info, pf=None):
    K1, K2, _ = case.shape
    e = TABLE[case.shape]
    assert info[0] == WLDS, f"{case}: expected dense_wlds_kernel, the hook says kernel {info[0]}"
    got = dict(tw=info[1], waves=info[2], chunks=chunks_of(K1, K2, info[3]), tp=info[4], nt=info[5], pf=info[6])
    want = dict(e, pf=e["pf"] if pf is None else pf)
    assert got == want, f"{case}: route {got}, the table says {want}"


def sweep(shape, N, expect, x_off=0, out_off=0, variants=VARIANTS):
    import torch
    for kind in ("exact", "gauss"):
        for (layout, pad, bias, act) in variants:
            c = Case(shape, N, kind, layout, pad, bias, act, x_off=x_off)
            y, info = c.run(out_off)
            expect(c, info)
            check(c, kind, y, f"pad={pad} bias={bias} x_off={x_off} out_off={out_off} {kind}")
            y2, _ = c.run(out_off)
            assert torch.equal(y, y2), f"{c}: not run-to-run identical"


def derived_rows(shape):
    """32 * CUs * waves * 2 + 32 * 3 + 7, waves from the hook after a probe call at N = 256"""
    import torch
    _, info = Case(shape, 256, "exact").run()
    assert info[0] == WLDS
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    return 32 * cus * info[2] * 2 + 32 * 3 + 7


# ---- dense_wlds_kernel ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=ident)
def test_threshold_and_ragged_rows(gm, shape):
    """N = 255 is dense_mfma_kernel's, 256 dense_wlds_kernel's with the table's configuration; 293 rows end in a 5-row tile"""
    def expect(c, info):
        if c.N < 256:
            assert info[0] == MFMA, f"{c}: expected dense_mfma_kernel, the hook says kernel {info[0]}"
        else:
            expect_wlds(c, info)
    for N in SMALL_ROWS:
        sweep(shape, N, expect)


@pytest.mark.parametrize("shape", LARGE_SHAPES, ids=ident)
def test_waves_with_two_and_three_tiles(gm, shape):
    """the persistent tile loop: second and third tiles of a wave, the prefetch hand-over full -> full and full -> ragged"""
    N = derived_rows(shape)
    sweep(shape, N, expect_wlds, variants=[VARIANTS[1], VARIANTS[6]])


@pytest.mark.parametrize("shape", PREFETCH_SHAPES, ids=ident)
def test_misaligned_x_and_out(gm, shape):
    """x one float into its buffer: still dense_wlds_kernel, prefetch and 16-byte staging off; out one float in: no 16-byte stores"""
    for N in (256 + 32 + 5, derived_rows(shape)):
        some = VARIANTS if N < 1000 else [VARIANTS[2], VARIANTS[5]]
        sweep(shape, N, lambda c, info: expect_wlds(c, info, pf=0), x_off=1, variants=some)
        sweep(shape, N, expect_wlds, out_off=1, variants=some)
        sweep(shape, N, lambda c, info: expect_wlds(c, info, pf=0), x_off=1, out_off=1, variants=some[:2])


@pytest.mark.parametrize("shape", PREFETCH_SHAPES + [(200, 0, 100), (257, 0, 100), (127, 127, 130)], ids=ident)
def test_scheduling_knob_does_not_change_a_bit(gm, shape):
    """knob 7: 17 = token + skew 1 (default), 0 = neither, 16 = token without skew, 49 = cross-tile prefetch off.  The kernel calls
    token and skew "performance only" and the prefetch only changes how x reaches LDS: identical bits."""
    import torch
    N = derived_rows(shape)
    for kind in ("exact", "gauss"):
        c = Case(shape, N, kind, 1, 1, 1, 1)
        y, info = c.run()
        expect_wlds(c, info)
        check(c, kind, y, f"knob 7 default {kind}")
        for v in (17, 0, 16, 49):
            with gm.tuned(gm.Knob.DENSE_PREFETCH, v):
                yv, info = c.run()
            expect_wlds(c, info, pf=0 if v == 49 else None)
            assert torch.equal(yv, y), f"{c}: knob 7 = {v} changes the result"


@pytest.mark.parametrize("shape", [(100, 0, 47), (200, 0, 100), (7, 0, 47)], ids=ident)     # whole-K (prefetch on), chunked, odd K
def test_non_finite_rows_stay_in_their_rows(gm, shape):
    """a NaN in the last real column of a row (next to odd K's zeroed column), an Inf in a wave's SECOND tile (a prefetched one where
    the prefetch is on), a -Inf row in the ragged last tile: exactly those output rows are non-finite, every other row keeps its bits"""
    import torch
    K1, _, _ = shape
    N = derived_rows(shape)
    c = Case(shape, N, "gauss", 0, 0, 1, 0)
    y, info = c.run()
    expect_wlds(c, info)
    second = 32 * (N // 32 // 2) + 32 * 5 + 9                 # a row of the second round of tiles
    rows = sorted([37, second, N - 3])
    x = c.xs[0]
    x[37, K1 - 1] = float("nan")
    x[second, K1 // 2] = float("inf")
    x[N - 3] = -float("inf")
    yb, info = c.run()
    expect_wlds(c, info)
    bad = ~torch.isfinite(yb).all(1)
    assert bad.nonzero().flatten().tolist() == rows
    assert torch.isnan(yb[37]).all() and not torch.isfinite(yb[second]).any() and not torch.isfinite(yb[N - 3]).any()
    assert torch.equal(yb[~bad], y[~bad])


# ---- dense_mfma_kernel ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES + MFMA_ONLY, ids=ident)
def test_k_chunked_kernel_forced(gm, shape):
    """knob 6 = 1: every product through dense_mfma_kernel (its 128 x 128 tiles end ragged in both directions at these sizes)"""
    def expect(c, info):
        assert info[0] == MFMA, f"{c}: expected dense_mfma_kernel, the hook says kernel {info[0]}"
    with gm.tuned(gm.Knob.DENSE_GENERIC, 1):
        for N in SMALL_ROWS:
            sweep(shape, N, expect)
        sweep(shape, SMALL_ROWS[-1], expect, x_off=1, out_off=1, variants=VARIANTS[:2])


@pytest.mark.parametrize("shape", MFMA_ONLY, ids=ident)
def test_k_chunked_kernel_by_default_when_w_does_not_fit_lds(gm, shape):
    def expect(c, info):
        assert info[0] == MFMA, f"{c}: expected dense_mfma_kernel, the hook says kernel {info[0]}"
    sweep(shape, 256 + 32 + 5, expect)


# ---- dense_narrow_kernel ----------------------------------------------------------------------------------------------------------
def expect_narrow(c, info):
    assert info[0] == NARROW, f"{c}: expected dense_narrow_kernel, the hook says kernel {info[0]}"


@pytest.mark.parametrize("Dout", range(1, 9))
def test_narrow_outputs(gm, Dout):
    """Dout 1..8 (all three instances), K a multiple of 4 above dense_t16's 128 so that Dout 4 and 8 arrive here too; one and two
    segments, both layouts, padded ldw; row counts that end inside a block's 32 rows"""
    for K1, K2 in ((132, 0), (136, 8), (4, 260)):
        for N in (1, 37, 256 + 32 + 5):
            sweep((K1, K2, Dout), N, expect_narrow)


def test_narrow_k_limit_and_alignment(gm):
    """K = 4096 is the last K the narrow kernel takes; 4100, or an x that is not 16-byte aligned, goes elsewhere"""
    def not_narrow(c, info):
        assert info[0] in (WLDS, MFMA), f"{c}: expected a matrix-core kernel, the hook says kernel {info[0]}"
    for Dout in (3, 8):
        sweep((4096, 0, Dout), 37, expect_narrow, variants=VARIANTS[:4])
        sweep((4100, 0, Dout), 37, not_narrow, variants=VARIANTS[:4])
        sweep((8, 4096, Dout), 37, expect_narrow, variants=VARIANTS[4:])
    for N in (37, 256 + 32 + 5):
        sweep((132, 0, 5), N, not_narrow, x_off=1)
        sweep((132, 0, 5), N, expect_narrow, out_off=1)


# ---- what the module as a whole has visited ---------------------------------------------------------------------------------------
def test_every_configuration_class_was_visited(gm):
    """from the hook's records, not from the table's comments: one probe per table shape here (so that the test stands alone), on top of
    whatever the tests above recorded"""
    for shape in SHAPES:
        Case(shape, 256, "exact").run()
    seen = {k: set() for k in ("nt", "tw", "waves", "chunks", "tp", "pf", "nseg")}
    for K1, K2, Dout, N, info in RECORDS:
        c = chunks_of(K1, K2, info[3])
        for k, v in (("nt", info[5]), ("tw", info[1]), ("waves", info[2]), ("chunks", min(c, 3)), ("tp", info[4]), ("pf", info[6]),
                     ("nseg", 2 if K2 else 1)):
            seen[k].add(v)
    assert seen["nt"] >= {1, 2, 3, 4}, seen
    assert seen["tw"] == {128, 64}, seen
    assert seen["waves"] == {8, 4}, seen
    assert seen["chunks"] == {1, 2, 3}, seen          # 3 stands for three or more
    assert seen["tp"] == {1, 2, 3, 4}, seen
    assert seen["pf"] == {0, 1}, seen
    assert seen["nseg"] == {1, 2}, seen
