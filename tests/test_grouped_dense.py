"""Grouped dense on the device against float64 numpy, group by group (tests/grouped_dense_cases.py).  Bounds are derived: an fp32 sum of n
products in any order is within n * 2^-24 of Σ|terms|, so the forward owes (K + 2) * 2^-24 * (Σ_k |x||W| + |b|) element-wise (as in
tests/test_dense_fallbacks.py) and ΔW (rows of the group + S) * 2^-24 * Σ_n |dz||x|: the slab's chain and the fold of S partials.  Integer
operands must come out exact: a row under another group's weight cannot hide under a tolerance.  Routes come from the debug export.
The launch geometries these shapes do not reach on a real device (several waves a super-tile, several super-tiles a block, S > 2 slabs,
...) are in tests/test_grouped_dense_geometry.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import evolve_ref as E  # noqa: E402
import grouped_dense_cases as GC  # noqa: E402

pytestmark = pytest.mark.gpu
U, SIZES = 2.0 ** -24, GC.SIZES
# (id, sizes, K, Dout, w_layout, bias, relu, strided): K's float4 tails, Dout's partial 16-block and two column tiles, one group, all empty but one, any-shape
FWD = [("k4", SIZES, 4, 12, 0, "group", 1, False), ("k20_strided", SIZES, 20, 12, 1, "shared", 0, True), ("k24", SIZES, 24, 12, 0, None, 0, False),
       ("k28", SIZES, 28, 12, 1, "group", 1, False), ("k100_d100", SIZES, 100, 100, 0, "shared", 0, False),
       ("d132_strided", SIZES, 20, 132, 1, "group", 1, True), ("one_group", (171,), 20, 12, 0, "shared", 1, False),
       ("one_nonempty", (0, 0, 0, 37, 0, 0), 20, 12, 0, "group", 0, False), ("any_2to3", SIZES, 2, 3, 1, "group", 0, True),
       ("any_5to7", SIZES, 5, 7, 0, "shared", 1, True)]
# (id, sizes, K, Dout, db, strided): one slab a group; two slabs on groups that are no multiple of four rows; the any-shape kernel
GRAD = [("mfma", SIZES, 20, 12, "group", True), ("mfma_two_slabs", (300, 0, 213), 24, 100, "shared", False), ("any_5x7", SIZES, 5, 7, "group", True),
        ("any_2x3", SIZES, 2, 3, "shared", False)]


dev = lambda a: None if a is None else __import__("torch").from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
draw = lambda rng, kind, *shape: (rng.integers(-3, 4, shape) if kind == "int" else rng.standard_normal(shape)).astype(np.float32)      # noqa: E731


def strided(a, ld, shift=0):
    import torch
    buf = torch.full((a.shape[0] * ld + shift + 4,), float("nan"), dtype=torch.float32, device="cuda")
    view = buf[shift:shift + a.shape[0] * ld].view(a.shape[0], ld)[:, :a.shape[1]]
    view.copy_(dev(a))
    return buf, view


def forward(x, W, b, seg, lay, relu, strd):
    import torch
    from gnnmp import grouped
    (N, K), G, Dout = x.shape, W.shape[0], W.shape[1 if lay == 0 else 2]
    pad, shift = ((4, 0) if K % 4 == 0 and Dout % 4 == 0 else (1, 1)) if strd else (0, 0)
    Wb = torch.full((G, Dout * K + 2 * pad), float("nan"), dtype=torch.float32, device="cuda")
    Wb[:, :Dout * K] = dev(W).view(G, -1)
    obuf, ov = strided(np.full((N, Dout), np.nan, np.float32), Dout + 2 * pad, shift)
    grouped.grouped_launch(strided(x, K + pad)[1], K + pad, Wb, Dout * K + 2 * pad, K if lay == 0 else Dout, lay, dev(b),
                           Dout if b is not None and b.ndim == 2 else 0, dev(seg), relu, ov, Dout + 2 * pad, N, G, K, Dout)
    out = ov.cpu().numpy()
    ov.fill_(float("nan"))
    assert torch.isnan(obuf).all(), "something was written between or around the rows of out"
    return out, grouped.last_route()


@pytest.mark.parametrize("case", FWD, ids=[c[0] for c in FWD])
def test_forward_against_float64(case):
    import gnnmp
    from gnnmp import grouped
    _, sizes, K, Dout, lay, bias, relu, strd = case
    seg, N, G = GC.seg_of(sizes), sum(sizes), len(sizes)
    want = grouped.ROUTE_T16 if K % 4 == 0 and Dout % 4 == 0 else grouped.ROUTE_FMA
    for kind in ("gauss", "int"):
        rng = np.random.default_rng(K * 1000 + Dout)
        x, W = draw(rng, kind, N, K), draw(rng, kind, G, *((Dout, K) if lay == 0 else (K, Dout)))
        b = None if bias is None else draw(rng, kind, *((G, Dout) if bias == "group" else (Dout,)))
        got, route = forward(x, W, b, seg, lay, relu, strd)
        assert route[0] == want and (want != grouped.ROUTE_T16 or route[1] == {12: 2, 100: 7, 132: 8}[Dout]), route
        bound = (K + 2) * U * GC.forward64(np.abs(x), np.abs(W), seg, None if b is None else np.abs(b), 0, lay)
        err = np.abs(got - GC.forward64(x, W, seg, b, relu, lay))
        assert np.all(err <= (bound if kind == "gauss" else 0.0)), f"{kind}: {int((err > 0).sum())} elements off, worst {err.max():.3e}"
        assert np.array_equal(forward(x, W, b, seg, lay, relu, strd)[0].view(np.uint32), got.view(np.uint32)), "two calls differ in bits"
    if G == 1:      # one group is gnnmp.dense (another summation order: both within the bound of the truth); the public form and its refusals
        tx, tW, tb = dev(x), dev(W), dev(b)
        assert np.array_equal(gnnmp.grouped_dense(tx, tW, [0, N], bias=tb, act="relu").cpu().numpy(), got)
        assert np.all(np.abs(gnnmp.dense(tx, tW[0], tb, "relu").cpu().numpy().astype(np.float64) - got) <= 2 * bound)
        for bad in ((tx, tW, [0, 100, N]), (tx[:, :8], tW, [0, N]), (tx, tW, [0, N], tb[:5]), (tx, tW.expand(2, Dout, K), [0, N, 100])):
            with pytest.raises(ValueError, match="seg_ptr has 3 entries|x has 8 columns, W contracts over 20|bias has shape|never decrease"):
                gnnmp.grouped_dense(*bad)


@pytest.mark.parametrize("case", GRAD, ids=[c[0] for c in GRAD])
def test_weight_gradient_against_float64(case):
    import torch
    from gnnmp import grouped
    _, sizes, K, Dout, db_mode, strd = case
    seg, N, G, rows = GC.seg_of(sizes), sum(sizes), len(sizes), np.array(sizes, np.float64)
    want = grouped.ROUTE_GRADW16 if K % 4 == 0 and Dout % 4 == 0 else grouped.ROUTE_GRADW_FMA
    pad = (4 if want == grouped.ROUTE_GRADW16 else 1) if strd else 0
    for kind in ("gauss", "int"):
        rng = np.random.default_rng(K * 1000 + Dout + 1)
        dz, x = draw(rng, kind, N, Dout), draw(rng, kind, N, K)

        def run():
            dW = torch.full((G, Dout * K + pad), float("nan"), device="cuda")
            db = torch.full((G, Dout) if db_mode == "group" else (Dout,), float("nan"), device="cuda")
            grouped.grouped_grad_launch(strided(dz, Dout + pad)[1], Dout + pad, strided(x, K + pad)[1], K + pad, dev(seg), dW, Dout * K + pad, db,
                                        Dout if db_mode == "group" else 0, N, G, K, Dout)
            assert pad == 0 or torch.isnan(dW[:, Dout * K:]).all()
            return dW[:, :Dout * K].reshape(G, Dout, K).cpu().numpy(), db.cpu().numpy(), grouped.last_route()
        dW, db, (kernel, S, _, _) = run()
        assert kernel == want and S == (2 if case[0] == "mfma_two_slabs" else 1), (kernel, S)
        (rW, rb), (mW, mb) = GC.grad64(dz, x, seg, db_mode == "shared"), GC.grad64(np.abs(dz), np.abs(x), seg, db_mode == "shared")
        bW, bb = (rows + S)[:, None, None] * U * mW, ((rows + S)[:, None] if db_mode == "group" else N + G * S) * U * mb
        assert np.all(np.abs(dW - rW) <= (bW if kind == "gauss" else 0.0)) and np.all(np.abs(db - rb) <= (bb if kind == "gauss" else 0.0)), kind
        assert not dW[rows == 0].any() and (db_mode == "shared" or not db[rows == 0].any()), "an empty group's gradient is zeros, written"
        assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(run()[:2], (dW, db))), "two calls differ in bits"


@pytest.mark.parametrize("K,Dout,lay,bias,act", [(20, 12, 0, "group", "relu"), (5, 7, 1, "shared", None), (24, 100, 1, "group", None)])
def test_grouped_dense_ad_against_float64(K, Dout, lay, bias, act):
    _ad_against_float64(K, Dout, lay, bias, act, SIZES)


def test_grouped_dense_ad_against_float64_cut_multiwave():
    """Δx — the forward with W read transposed — and ΔW on super-tiles of four waves cut by boundaries (grouped_dense_cases.py: CUT)"""
    _ad_against_float64(24, 12, 0, "group", "relu", GC.CUT)


def _ad_against_float64(K, Dout, lay, bias, act, sizes):
    import gnnmp
    import torch
    seg, N, G, rows, rng = GC.seg_of(sizes), sum(sizes), len(sizes), np.array(sizes, np.float64), np.random.default_rng(K + Dout)
    x, W = draw(rng, "gauss", N, K), draw(rng, "gauss", G, *((Dout, K) if lay == 0 else (K, Dout)))
    b, dy = draw(rng, "gauss", *((G, Dout) if bias == "group" else (Dout,))), draw(rng, "gauss", N, Dout)
    tx, tW, tb = (dev(a).requires_grad_() for a in (x, W, b))
    y = gnnmp.grouped_dense_ad(tx, tW, dev(seg), bias=tb, act=act, w_layout=lay)
    assert torch.equal(y, gnnmp.grouped_dense(tx, tW, dev(seg), bias=tb, act=act, w_layout=lay))
    gx, gW, gb = (g.cpu().numpy() for g in torch.autograd.grad(y, [tx, tW, tb], dev(dy)))
    dz = dy * (y.detach().cpu().numpy() > 0) if act else dy.astype(np.float64)      # relu' of the y the kernel computed
    Wt = np.swapaxes(W, 1, 2)
    assert np.all(np.abs(gx - GC.forward64(dz, Wt, seg, None, 0, lay)) <= (Dout + 2) * U * GC.forward64(np.abs(dz), np.abs(Wt), seg, None, 0, lay))
    (rW, rb), (mW, mb) = GC.grad64(dz, x, seg, bias == "shared"), GC.grad64(np.abs(dz), np.abs(x), seg, bias == "shared")
    if lay == 1:
        rW, mW = np.swapaxes(rW, 1, 2), np.swapaxes(mW, 1, 2)
    assert np.all(np.abs(gW - rW) <= (rows + 1)[:, None, None] * U * mW) and np.all(np.abs(gb - rb) <= ((rows + 1)[:, None] if bias == "group" else N + G) * U * mb)


@pytest.mark.parametrize("c", E.LAYER_CASES, ids=E.case_id)
def test_evolve_gcno_grouped_against_float64(c):
    import gnnmp
    import torch
    import test_evolve_gcno as EG
    case, ys64, _, g64 = EG.reference(c)
    tg, layer, plain = EG.make_tg(case["snaps"]), EG.make_layer(c, case), EG.make_layer(c, case)
    assert plain.cell.grouped is False and not setattr(layer.cell, "grouped", True)
    xs = [EG.dev(x).requires_grad_() for x in case["xs"]]
    st = None if case["state"] is None else [EG.dev(a).requires_grad_() for a in case["state"]]
    params = {k: p.requires_grad_() for k, p in zip(["conv_w", "conv_b", "Wi", "Wh", "b"], layer.cell.parameters()) if p is not None}
    ys = gnnmp.evolve_gcno_ad(layer, tg, xs, None if st is None else (st[0], (st[1], st[2])))
    for t, (y, ref) in enumerate(zip(ys, ys64)):
        EG.close(y, ref, f"y[{t}]")
    wrt = {f"x{t}": x for t, x in enumerate(xs)}
    wrt.update({k: v for k, v in params.items() if not (k == "conv_w" and st is not None)})
    wrt.update({} if st is None else dict(zip(("weight", "h", "c"), st)))
    for k, gr in zip(wrt, torch.autograd.grad(sum((y * EG.dev(dy)).sum() for y, dy in zip(ys, case["dys"])), list(wrt.values()))):
        EG.close(gr, g64[k], f"d{k}")
    with torch.no_grad():
        det, xd = None if st is None else (st[0].detach(), (st[1].detach(), st[2].detach())), [x.detach() for x in xs]
        layer.cell.grouped = False                            # the flag is the only switch: off, the layer is the default layer again
        assert all(torch.equal(u, v) for u, v in zip(plain(tg, xd, det), layer(tg, xd, det)))


@pytest.mark.parametrize("ch", [(3, 5), (5, 3), (8, 8)], ids=["aggregate_first", "w_first", "mfma"])
def test_evolve_gcno_grouped_launch_count(monkeypatch, ch):
    import gnnmp
    import test_evolve_gcno as EG
    from gnnmp import _lib
    layers = {True: gnnmp.EvolveGCNO(ch, seed=2, grouped=True), False: gnnmp.EvolveGCNO(ch, seed=2)}
    tgs = {T: EG.make_tg(E.snapshots(ch[0], T, 2)) for T in (2, 5)}
    xs = {T: [EG.dev(np.zeros((n, ch[0]), np.float32)) for n in tgs[T].num_nodes] for T in tgs}
    for T in tgs:
        layers[True](tgs[T], xs[T])                           # the batch, its plan, its normalisation and its boundaries are made once
    proxy, counts = EG._Counting(_lib.load()), {}
    monkeypatch.setattr(_lib, "_lib", proxy)
    for grouped, T in ((g, T) for g in layers for T in tgs):
        proxy.calls.clear()
        layers[grouped](tgs[T], xs[T])
        counts[grouped, T] = list(proxy.calls)
    monkeypatch.undo()
    for T in tgs:
        assert counts[True, T].count("gnnmp_grouped_dense_f32") == 1 and "gnnmp_dense_f32" not in counts[True, T], counts[True, T]
        assert counts[False, T].count("gnnmp_dense_f32") == T and "gnnmp_grouped_dense_f32" not in counts[False, T]
    assert len(counts[True, 5]) - len(counts[True, 2]) == 3
