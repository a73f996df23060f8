"""gnnmp_topk_select_radix_f32 (csrc/topk.hip) against tests/topk_ref.py's `select`, word for word.  The cases register in the table of
tests/abi_cases.py (as tests/topk_cases.py does): keep and workspace come from its poisoned, guarded slab, and its capture check applies."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_cases as A  # noqa: E402
import topk_ref as R  # noqa: E402

gpu = pytest.mark.gpu
NAME, WORKSPACE = "gnnmp_topk_select_radix_f32", "gnnmp_topk_select_radix_workspace"
TILE = int(A.parse_header()[1]["GNNMP_TOPK_RADIX_TILE"])
# no large graph starts or ends on a tile boundary; tile 2 holds the tail of a tiled graph, an empty graph and the head of the next
SIZES = (257, 2 * TILE + 1, 0, 5000, 1, TILE + 1, 255, TILE, 1030, 256)
HI, MID, K_FIRST, K_LAST = 40, 150, 41, 190      # "three": HI nodes of a graph hold the top value, MID the middle one, the rest the lowest
KS = ((1, 0.0), (6000, 0.0), (0, 0.5), (K_FIRST, 0.0), (K_LAST, 0.0))
KINDS = ("gauss", "three", "equal", "specials", "low8", "top8")
# (tag, member sizes | None: one graph, N, count_nodes, lds_nodes, (k, ratio) list, kinds); K_FIRST / K_LAST put rank k - 1 on the first /
# the last node of "three"'s middle tie group, which spreads over tiles and waves in the large members (checked when the cases were made)
LAYOUTS = (("batch", SIZES, sum(SIZES), 256, TILE, KS, KINDS), ("one5000", None, 5000, 256, TILE, KS[2:4], KINDS),
           ("one300", None, 300, 256, TILE, KS[2:4], KINDS), ("defaults", SIZES, sum(SIZES), 0, 0, KS[2:3], ("three",)),
           ("count16", R.SIZES, sum(R.SIZES), 16, TILE, KS[2:3], ("three",)))      # several LDS-route graphs start in one 256-node tile


def scores(kind, r, ptr):
    N = int(ptr[-1])
    if kind == "gauss":                 # distinct Gaussians (Box-Muller on the table's uniform draws: they differ between the variants)
        return (np.sqrt(-2.0 * np.log(1.0 - r.random(N))) * np.cos(2.0 * np.pi * r.random(N))).astype(np.float32)
    if kind == "three":
        out = np.empty(N, np.float32)
        for a, b in zip(ptr[:-1], ptr[1:]):
            out[a:b] = np.array([0.5] * HI + [0.25] * MID + [-1.0] * max(0, b - a - HI - MID), np.float32)[: b - a][r.permutation(b - a)]
        return out
    if kind == "equal":
        return np.full(N, 0.25, np.float32)
    if kind == "specials":              # NaNs of both signs, +-0.0, +-Inf, subnormals
        return R.score_vectors(ptr)["specials"]
    if kind == "low8":                  # the top 24 bits agree: only the last pass decides
        return (np.uint32(0x3f800000) | r.integers(0, 256, N).astype(np.uint32)).view(np.float32)
    return ((r.integers(0, 256, N).astype(np.uint32) << np.uint32(24)) | np.uint32(0x00345678)).view(np.float32)      # top8: finite


def build(ctx):
    n = 0
    for tag, sizes, N, count_nodes, lds_nodes, ks, kinds in LAYOUTS:
        ptr = None if sizes is None else R.batch_ptr(sizes)
        for kind in kinds:
            for k, ratio in ks:
                for ties in (R.FIRST, R.ALL):
                    n += 1
                    ib = 4 << (n % 2)
                    y = scores(kind, A.rng_of("topk_radix", tag, kind), np.array([0, N]) if ptr is None else ptr)
                    nbytes = (N + TILE - 1) // TILE * (2 * 256 + 4) * 4 if N > TILE and lds_nodes else 0      # (the defaults need none here)
                    first = (tag, kind, k, ties) == ("batch", "gauss", 0, R.FIRST)
                    job = A.Rec("gnnmp_topk_radix_t", score=A.Arr("score", "in", y),
                                graph_ptr=None if ptr is None else A.Arr("graph_ptr", "in", ptr.astype(np.int64 if ib == 8 else np.int32)),
                                idx_bytes=ib, n_graphs=1 if ptr is None else len(ptr) - 1, k=k, ratio=ratio, ties=ties, count_nodes=count_nodes,
                                lds_nodes=lds_nodes, keep=A.Arr("keep", "out", shape=(N + 1,), dtype=np.uint32),
                                workspace=A.Arr("workspace", "scratch", shape=(nbytes // 4,), dtype=np.uint32) if nbytes else None,
                                workspace_bytes=nbytes)
                    yield A.mk(NAME, f"{tag}_{kind}_k{k}_r{ratio}_t{ties}_i{ib}", {"align", "side"} if first else (), [job, N, A.STREAM],
                               lambda host, v=(y, ptr, k, ratio, ties): {"keep": A.E(R.select(*v)[0], "exact")}, no_warmup=True)


if NAME not in A.TABLE:
    A.TABLE[NAME] = A._of_variant(build)
THR = int(A.parse_header()[1]["GNNMP_MIN_LONG_ROW"])
CASES = A.TABLE[NAME](A.Ctx(THR))


@pytest.fixture(scope="module")
def lib():
    from gnnmp import _lib
    return _lib.load()


def test_header_symbols_library_and_record():
    from gnnmp import _lib
    h = A.parse_header()
    nm = os.popen(f"nm -D --defined-only {_lib.LIB_PATH}").read()
    for name in (NAME, WORKSPACE):
        assert name in h[0] and name in _lib.SYMBOLS and f" T {name}\n" in nm, name
    st = A.struct_of("gnnmp_topk_radix_t")
    assert st is _lib.TopkRadixJob and _lib.TOPK_RADIX_TILE == TILE and [p[0] for p in h[0][NAME]] == ["job", "N", "stream"]
    assert [n for n, _ in st._fields_] == [f[0] for f in h.records["gnnmp_topk_radix_t"]] == [
        "score", "graph_ptr", "idx_bytes", "n_graphs", "k", "ratio", "ties", "count_nodes", "lds_nodes", "keep", "workspace", "workspace_bytes"]
    assert dict(st._fields_)["ratio"] is ctypes.c_float and ctypes.sizeof(st) == 88 and ctypes.sizeof(_lib.TopkJob) == 72
    texts = " ".join(A.header_comments_of(NAME))
    assert "pool.jl:14-27" in texts and "SAME WORDS" in texts and not A.WAITS_OR_ALLOCATES.search(texts) and NAME in A.capturable()


P_ = lambda v: ctypes.c_void_p(0x1000 * v) if v else None      # never dereferenced: the call must refuse first  # noqa: E731


def test_refusals_and_workspace_size_need_no_device(lib):
    from gnnmp import _lib
    EINVAL, err, ws_of = _lib.EINVAL, lib.gnnmp_last_error, lib.gnnmp_topk_select_radix_workspace

    def select(job=True, score=1, gp=None, ib=8, G=1, k=4, ratio=0.0, ties=0, cn=0, ln=0, keep=2, ws=3, wb=1 << 40, N=10):
        j = _lib.TopkRadixJob(P_(score), P_(gp), ib, G, k, ratio, ties, cn, ln, P_(keep), P_(ws), wb)
        return lib.gnnmp_topk_select_radix_f32(ctypes.byref(j) if job else None, N, None)

    assert select(job=False) == EINVAL and b"null job" in err()
    assert select(N=-1) == EINVAL and b"negative N" in err()
    assert select(N=2 ** 31 - 1) == _lib.EUNSUPPORTED
    for kw, word in ((dict(ib=0), b"idx_bytes"), (dict(ib=16), b"idx_bytes"), (dict(gp=3, G=0), b"n_graphs"), (dict(k=-1), b"k = -1"),
                     (dict(k=0, ratio=0.0), b"ratio"), (dict(k=0, ratio=1.5), b"ratio"), (dict(k=0, ratio=float("nan")), b"ratio"),
                     (dict(ties=2), b"ties"), (dict(ties=-1), b"ties"), (dict(cn=-1), b"count_nodes"), (dict(ln=-1), b"lds_nodes"),
                     (dict(keep=None), b"null keep"), (dict(score=None), b"null score"),
                     (dict(N=20000, ws=None), b"workspace"), (dict(N=20000, wb=ws_of(20000) - 1), b"workspace"),
                     (dict(N=5000, ln=TILE, wb=ws_of(5000) - 4), b"workspace")):
        assert select(**kw) == EINVAL and word in err(), kw
    sizes = [ws_of(N) for N in (0, 1, TILE, TILE + 1, 2 * TILE, 2 * TILE + 1, 169343, 2 ** 31 - 2)]
    assert sizes[:3] == [0, 0, 0] and sizes[3] == 2 * (2 * 256 + 4) * 4 == sizes[4] and sizes == sorted(sizes) and sizes[6] == 83 * 2064


@gpu
@pytest.mark.parametrize("case", CASES, ids=[c.sid for c in CASES])
def test_equal_words(lib, case):
    """keep == the reference's words, keep[N] = 0, every word written, nothing outside keep and workspace, from a poisoned workspace"""
    rc, slab, host = A.run_case(lib, case, None)
    assert not A.verify(case, rc, slab, host), A.verify(case, rc, slab, host)


@gpu
def test_capture_cold_replay_new_scores(lib):
    """recorded with a poisoned workspace and no eager call first, replayed on other scores at the same addresses, twice back to back"""
    import torch
    import test_abi_graph_capture as C
    C._require_working_capture()
    (c0,), (c1,) = (C._capture_cases(A.Ctx(THR, variant=v), NAME) for v in (0, 1))
    assert c0.no_warmup
    problems = C._record_and_replay(lib, c0, c1, None, torch.cuda.Stream())
    assert not problems, "\n".join(problems)


@gpu
def test_pool_and_index_reach_it_and_the_routes_agree():
    """route = "auto" on a batch with a 5000-node member: the restatement's kept nodes, child edges, x2; "count" == "radix" """
    import torch
    import gnnmp as gm
    from gnnmp import pool_topk as PT
    from test_topk_pool import _dev, _exact_batch, _np, close
    g, h = _exact_batch(gm, sizes=(9, 5000, 300, 0, 2500))
    p = np.array([1, 1, 1, 1, 0, 0, 0], np.float32)
    l = gm.TopKPool(0.5, 7, act="tanh")
    l.p = _dev(p)
    idx0, x2_ref, s2, t2, eid = R.topk_pool(h["x"], p, h["s0"], h["t0"], h["ptr"], 0, 0.5, R.TANH)
    g2, x2 = gm.topk_pool(l, g, g.x)
    assert all(np.array_equal(_np(a), b + 1) for a, b in ((g2.nid, idx0), (g2.s, s2), (g2.t, t2), (g2.eid, eid)))
    close(_np(x2), x2_ref, "x2")
    y = PT.topk_score(g.x, l.p)
    assert np.array_equal(_np(gm.topk_index(y, 0.3, g)), np.flatnonzero(R.select(_np(y), h["ptr"], 0, 0.3, R.ALL)[0]) + 1)
    for ties in ("first", "all"):
        kc, kr, ka = (PT.topk_select(y, 0, 0.5, g, ties, route=r, **kw)[0]
                      for r, kw in (("count", {}), ("radix", dict(lds_nodes=TILE)), ("auto", {})))
        assert torch.equal(kc, kr) and torch.equal(kc, ka)
