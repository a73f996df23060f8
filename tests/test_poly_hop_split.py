"""The split route of the hop (csrc/poly_conv.hip, csrc/slotwalk.h; include/gnnmp.h states the arithmetic and the fold order) on one 400-node
graph with rows at, just above and far above the plan's threshold.  The export writes through its record and its workspace, so its cases
register in the table of tests/abi_cases.py (as tests/test_topk_radix.py does) and run in its poisoned, guarded slab.
THE ELEMENT-WISE BOUND.  A term w ss z of row i passes through at most 2 products (ss, w), len_i additions (its chunk's, then the fold's:
never more than the row has slots), the products by scale_dst and alpha and 3 epilogue additions; beta self and gamma prev carry fewer.
So |got - ref64| <= γ_n Σ|terms|, n = len_i + 8 (γ_n: tests/megnet_conv_ref.py), whatever the grouping of the sum."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_cases as A  # noqa: E402
import poly_conv_ref as R  # noqa: E402

gpu = pytest.mark.gpu
f32, f64 = np.float32, np.float64
NAME, WHOLE, QUERY = "gnnmp_poly_hop_split_f32", "gnnmp_poly_hop_ld_f32", "gnnmp_poly_hop_split_workspace"
THR = int(A.parse_header()[1]["GNNMP_MIN_LONG_ROW"])      # the threshold of a plan this small; the GPU tests assert plan.long_thresh == THR
N, HUB_IN, AT_T, OVER_T, NO_IN, HUB_OUT = 400, 7, 8, 9, 3, 11
DS, KINDS = (1, 5, 64, 100, 260), ("plain", "scaled", "panel")


def edges():
    """(s, t) 0-based, shuffled: HUB_IN 300 in-edges from 37 repeating sources, AT_T exactly THR, OVER_T THR + 1, NO_IN none, HUB_OUT 300
    out-edges (one to each of 100 .. 399), every other node 0 - 3 in-edges"""
    rng = np.random.default_rng(2611)
    deg = rng.integers(0, 3, N)                                     # + HUB_OUT's edge: at most 3
    deg[[HUB_IN, AT_T, OVER_T, NO_IN]] = 0
    t = np.concatenate([np.repeat(np.arange(N), deg), np.full(300, HUB_IN), np.full(THR, AT_T), np.full(THR + 1, OVER_T), np.arange(100, 400)])
    s = np.concatenate([rng.integers(12, 100, int(deg.sum())), 20 + np.arange(300) % 37, 100 + np.arange(THR), 100 + np.arange(THR + 1), np.full(300, HUB_OUT)])
    p = rng.permutation(len(s))
    return s[p].astype(np.int64), t[p].astype(np.int64)


S0, T0 = edges()
G = A.Graph("hub400", S0 + 1, T0 + 1, N)


def chunks(rows):
    """the plan's chunk count: a row longer than THR is cut into ceil(len / min(THR, 128)) chunks (csrc/plan.hip)"""
    return int(sum(-(-int(v) // min(THR, 128)) for v in np.bincount(rows, minlength=N) if v > THR))


def operands(D, T, kind, r):
    """(s, t, ops float32 per edge / node, coef) of a case; T: over the transposed plan"""
    s, t = (T0, S0) if T else (S0, T0)
    ops = dict(z=A.F(r, N, D))
    if kind != "plain":
        ops.update(w=(1.0 + 0.5 * A.F(r, len(s))).astype(f32), ss=(1.0 + 0.5 * A.F(r, len(s))).astype(f32), sd=(1.0 + 0.5 * A.F(r, N)).astype(f32),
                   self_=A.F(r, N, D), prev=A.F(r, N, D), add=A.F(r, N, D))
    return s, t, ops, (R.ALPHA, R.BETA if kind != "plain" else 0.0, R.GAMMA if kind != "plain" else 0.0)


def hop64(s, t, ops, coef, absolute=False):
    """the float64 hop, or Σ|terms| of it"""
    c = (lambda v: np.abs(v.astype(f64))) if absolute else (lambda v: v.astype(f64))
    kw = {k: c(v) for k, v in ops.items() if k != "z"}
    return R.hop(s, t, N, c(ops["z"]), alpha=c(f64(coef[0])), beta=c(f64(coef[1])), gam=c(f64(coef[2])), **kw)


def build(ctx):
    for k, (D, T, kind) in enumerate((D, T, kind) for D in DS for T in (False, True) for kind in KINDS):
        r = A.rng_of("poly_hop_split", D, T, kind)
        s, t, ops, coef = operands(D, T, kind, r)
        order = np.argsort(t, kind="stable")
        slot = lambda nm, key: A.Arr(nm, "in", ops[key][order] if key in ("w", "ss") else ops[key]) if key in ops else None      # noqa: E731
        f = dict(z=A.Arr("z", "in", ops["z"]), w_slot=slot("w_slot", "w"), ss_slot=slot("ss_slot", "ss"), scale_dst=slot("scale_dst", "sd"),
                 self=slot("self", "self_"), prev=None, add=slot("add", "add"))
        ld = dict.fromkeys(("z", "self", "prev", "add", "out"), D)
        want = hop64(s, t, ops, coef)
        if kind == "panel":                     # z, prev, add and out are column blocks of one panel; self keeps a buffer of its own
            w = 4 * D + 3
            cols = dict(z=1, prev=D + 1, add=2 * D + 2, out=3 * D + 3)
            pan, om = A.F(r, N, w), np.zeros((N, w), bool)
            for nm in ("z", "prev", "add"):
                pan[:, cols[nm]:cols[nm] + D] = ops[nm]
            om[:, cols["out"]:cols["out"] + D] = True
            pan[om] = np.nan
            P = A.Arr("panel", "inout", pan)
            f.update({nm: A.Arr(nm, "in", base=P, offset=cols[nm]) for nm in ("z", "prev", "add")})
            out, name, full = A.Arr("out", "out", base=P, offset=cols["out"]), "panel", np.zeros((N, w))
            full[om] = want.reshape(-1)
            ref = lambda host, a=(pan, om, full): {"panel": A.part_E(*a)}      # noqa: E731
            ld.update(z=w, prev=w, add=w, out=w)
        elif kind == "scaled":                  # prev == out, in place
            both = A.Arr("prev_out", "inout", ops["prev"])
            f["prev"], out, name, om = A.Arr("prev", "in", base=both), A.Arr("out", "out", base=both), "prev_out", None
            ref = lambda host, want=want: {"prev_out": want}      # noqa: E731
        else:
            out, name, om = A.Arr("out", "out", shape=(N, D)), "out", None
            ref = lambda host, want=want: {"out": want}      # noqa: E731
        job = A.Rec("gnnmp_poly_hop_ld_t", **f, alpha=coef[0], beta=coef[1], gamma=coef[2], out=out, ld_z=ld["z"], ld_self=ld["self"],
                    ld_prev=ld["prev"], ld_add=ld["add"], ld_out=ld["out"])
        nws = chunks(t) * D
        tags = {0: {"side", "align"}, 1: {"ws"}, 8: {"align"}}.get(k, set())
        c = A.mk(NAME, f"D{D}_{'T' if T else 'P'}_{kind}", tags, [A.Pl(G, T=T), job, D, A.Arr("workspace", "scratch", shape=(nws,)), 4 * nws, A.STREAM],
                 ref, no_warmup=True)
        c.whole = A.mk(WHOLE, c.sid, (), [A.Pl(G, T=T), job, D, A.STREAM], ref, no_warmup=True)
        c.bound = (name, om, want, R.gamma(np.bincount(t, minlength=N)[:, None] + 8.0) * hop64(s, t, ops, coef, True), np.bincount(t, minlength=N) <= THR)
        yield c


if NAME not in A.TABLE:
    A.TABLE[NAME] = A._of_variant(build)
CASES = A.TABLE[NAME](A.Ctx(THR))


@pytest.fixture(scope="module")
def lib():
    from gnnmp import _lib
    return _lib.load()


def test_header_symbols_library_and_wrappers():
    import torch
    from gnnmp import _lib, backward_poly as B
    h = A.parse_header()
    nm = os.popen(f"nm -D --defined-only {_lib.LIB_PATH}").read()
    for name in (NAME, QUERY):
        assert name in h[0] and name in _lib.SYMBOLS and f" T {name}\n" in nm, name
    assert [p[0] for p in h[0][NAME]] == ["plan", "job", "D", "workspace", "workspace_bytes", "stream"] and h[0][NAME][1][2]
    texts = " ".join(A.header_comments_of(NAME))
    assert "Launch-only, capturable" in open(A.HEADER).read() and "IN CHUNK ORDER" in texts and not A.WAITS_OR_ALLOCATES.search(texts) and NAME in A.capturable()
    assert np.bincount(T0, minlength=N)[[HUB_IN, AT_T, OVER_T, NO_IN]].tolist() == [300, THR, THR + 1, 0] and np.bincount(S0)[HUB_OUT] == 300
    assert sorted(np.flatnonzero(np.bincount(T0, minlength=N) > THR)) == [HUB_IN, OVER_T] and np.bincount(T0, minlength=N).max() == 300
    with pytest.raises(ValueError, match="route 'chunks'"):
        B.poly_hop(None, torch.zeros(2, 2), 1.0, route="chunks")


@gpu
@pytest.mark.parametrize("case", CASES, ids=[c.sid for c in CASES])
def test_hop_split(lib, case):
    """every owed element inside γ_n Σ|terms| and 1e-5 of float64; everything else of the slab — inputs, the panel's other columns, the
    guards around out and around the n_chunks * D floats of the workspace — untouched; rows of at most THR slots have the whole route's
    bits; a second call gives equal bits"""
    plans = A.Plans(lib)
    try:
        info, need = (ctypes.c_int64 * 8)(), ctypes.c_int64(-1)
        plan = plans.get(case.args[0])
        assert lib.gnnmp_plan_info(plan, info) == A.OK and info[7] == THR and info[5] == (1 if case.args[0].T else 2)      # plan.n_long == 2, plan_t.n_long >= 1
        assert lib.gnnmp_poly_hop_split_workspace(plan, case.args[2], ctypes.byref(need)) == A.OK and need.value == case.args[4] > 0
        runs = []
        for c in (case, case, case.whole):
            rc, slab, host = A.run_case(lib, c, plans)
            assert not A.verify(c, rc, slab, host), (c.export, A.verify(c, rc, slab, host))
            runs.append(slab.outputs())
    finally:
        plans.close()
    name, om, want, bound, short = case.bound
    got, again, whole = (o[name].view(f32).reshape(N, -1) for o in runs)
    if om is not None:
        got, again, whole = (v[om].reshape(N, -1) for v in (got, again, whole))
    err = np.abs(got.astype(f64) - want)
    print(f"{case.sid}: uses {float((err / np.maximum(bound, 1e-300)).max()):.3f} of the summation bound")
    assert np.all(err <= bound)
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32)), "two calls differ"
    assert np.array_equal(got[short].view(np.uint32), whole[short].view(np.uint32)), "a row the plan does not split lost the whole route's bits"


@gpu
@pytest.mark.parametrize("bad", ["small", "null", "overlap"])
def test_refusals_write_nothing(lib, bad):
    """a workspace one float too small, a NULL workspace with split rows, a workspace that overlaps out: GNNMP_EINVAL, every buffer as poisoned"""
    from gnnmp import _lib
    case = CASES[3]
    plans = A.Plans(lib)
    try:
        slab = A.Slab(case.arrs, "cuda", None, case.guard)
        cargs, _ = A.bind(case, slab, plans, None)
        cargs = list(cargs)
        if bad == "small":
            cargs[4] -= 4
        elif bad == "null":
            cargs[3] = None
        else:
            cargs[3] = ctypes.c_void_p(slab.ptr("out").value + 4 * (N * case.args[2] - 1))       # its first float is out's last
        assert getattr(lib, NAME)(*cargs) == _lib.EINVAL and b"poly_hop_split: " in lib.gnnmp_last_error() and b"workspace" in lib.gnnmp_last_error()
        assert not slab.check({}, untouched=True)
    finally:
        plans.close()


@gpu
def test_capture_without_an_eager_call(lib):
    """recorded cold with a poisoned workspace, replayed on other values at the same addresses, compared bit for bit with eager calls"""
    import torch
    import test_abi_graph_capture as C
    C._require_working_capture()
    for c0, c1 in zip(C._capture_cases(A.Ctx(THR, variant=0), NAME), C._capture_cases(A.Ctx(THR, variant=1), NAME)):
        plans = A.Plans(lib)
        try:
            problems = C._record_and_replay(lib, c0, c1, plans, torch.cuda.Stream())
        finally:
            plans.close()
        assert c0.no_warmup and not problems, "\n".join(problems)


def layer_graph(bidirected):
    """the hop graph; bidirected: its distinct undirected pairs and a ring (no isolated node), once in each direction"""
    if not bidirected:
        return S0, T0
    a, b = np.concatenate([S0, np.arange(N)]), np.concatenate([T0, (np.arange(N) + 1) % N])
    pairs = np.unique(np.stack([np.minimum(a, b), np.maximum(a, b)], 1)[a != b], axis=0)
    return np.concatenate([pairs[:, 0], pairs[:, 1]]), np.concatenate([pairs[:, 1], pairs[:, 0]])


@gpu
@pytest.mark.parametrize("layer", ["cheb", "dconv", "gconv_gru"])
def test_layers_take_the_split_route(layer):
    """cheb_conv_ad (k = 3), d_conv_ad (k = 2) at 8 => 8 and gconv_gru_ad (T = 2, k = 2, 3 => 4): forward and every gradient within 1e-5
    of float64, norm-wise and element-wise (tests/test_poly_conv_ad.py: close); every hop took the split route"""
    import torch
    import gnnmp
    import recurrent_ref as RR
    from gnnmp import backward_poly as B
    from test_poly_conv_ad import close, dev
    s, t = layer_graph(layer != "dconv")
    g = gnnmp.GNNGraph(dev(s), dev(t), num_nodes=N, index_base=0)
    assert g.plan(False).n_long >= 1 and g.plan_transposed(False).n_long >= 1
    rng = np.random.default_rng([2612, len(layer)])
    before = dict(B.ROUTES_TAKEN)
    if layer == "gconv_gru":
        l = gnnmp.GConvGRU((3, 4), 2, bias=True, seed=1)
        params = [p.requires_grad_() for p in l.cell.parameters()]
        x, dy = rng.standard_normal((N, 2, 3)).astype(f32), rng.standard_normal((N, 2, 4)).astype(f32)
        xt = dev(x).requires_grad_()
        y = gnnmp.gconv_gru_ad(l, g, xt)
        got = [y.detach()] + list(torch.autograd.grad(y, [xt] + params, dev(dy)))
        p64 = [p.detach().cpu().double().requires_grad_() for p in params]
        x64 = torch.from_numpy(x).double().requires_grad_()
        y64 = RR.scan("gconv_gru", RR.Graph(s, t, N, None, gnnmp.layers_more.scaled_laplacian_op(g)[3]), p64, x64, None)
        ref = [y64.detach()] + list(torch.autograd.grad(y64, [x64] + p64, torch.from_numpy(dy).double()))
    else:
        x, dy = rng.standard_normal((N, 8)).astype(f32), rng.standard_normal((N, 8)).astype(f32)
        xt = dev(x).requires_grad_()
        if layer == "cheb":
            W, b = np.stack([R.glorot(rng, 8, 8) for _ in range(3)]), (0.1 * rng.standard_normal(8)).astype(f32)
            l = gnnmp.ChebConv((8, 8), 3)
            l.weight, l.bias = dev(W).requires_grad_(), dev(b).requires_grad_()
            y, leaves = gnnmp.cheb_conv_ad(l, g, xt), [l.weight, l.bias]
            r = R.cheb_grad(s, t, N, x.astype(f64), W.astype(f64), b.astype(f64), gnnmp.layers_more.scaled_laplacian_op(g)[3], dy.astype(f64))
        else:
            W, b = np.stack([np.stack([R.glorot(rng, 8, 8) for _ in range(2)]) for _ in range(2)]), (0.1 * rng.standard_normal(8)).astype(f32)
            l = gnnmp.DConv((8, 8), 2)
            l.weights, l.bias = dev(W).requires_grad_(), dev(b).requires_grad_()
            y, leaves = gnnmp.d_conv_ad(l, g, xt), [l.weights, l.bias]
            r = R.dconv_grad(s, t, N, x.astype(f64), W.astype(f64), b.astype(f64), dy.astype(f64))
        got = [y.detach()] + list(torch.autograd.grad(y, [xt] + leaves, dev(dy)))
        ref = [r["Y"], r["dx"], r["dW"], r["db"]]
    torch.cuda.synchronize()
    assert B.ROUTES_TAKEN["split"] > before["split"] and B.ROUTES_TAKEN["whole"] == before["whole"]
    for k, (a, b_) in enumerate(zip(got, ref)):
        close(a.cpu().numpy(), np.asarray(b_), f"{layer}[{k}]")
