"""Grouped dense at the launch geometries a real device reaches (csrc/dense_grouped.hip, planned by csrc/dense_grouped_route.h): super-tiles
of several waves cut by group boundaries, blocks that own several super-tiles and walk several groups, every column-block instance and the
LDS step-down, the any-shape kernel over several blocks; the weight gradient with S > 2 slabs and groups shorter than 4 S rows, its MFMA
split over grid.y / grid.z / waves, both kernels without dW or db; non-finite values that must stay inside their group.  Cases:
tests/grouped_dense_cases.py (GEOM_FWD, GEOM_GRAD); references and bounds are those of tests/test_grouped_dense.py — integer operands
exact, gauss operands within (K + 2) * 2^-24 * forward64(|x|, |W|, |b|) and (rows + S) * 2^-24 * grad64(|dz|, |x|) — and every case
asserts from the route record that it reached the geometry it is named for (tests/test_grouped_route_cpu.py: what that is at 256 CUs)."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grouped_dense_cases as GC  # noqa: E402
import test_grouped_dense as T  # noqa: E402

pytestmark = pytest.mark.gpu
U, NAN, INF = 2.0 ** -24, np.float32("nan"), np.float32("inf")
dev, draw, strided = T.dev, T.draw, T.strided
bits = lambda a: np.ascontiguousarray(a).view(np.uint32)      # noqa: E731
# finite, +Inf, -Inf, NaN
klass = lambda a: np.where(np.isnan(a), 3, np.where(np.isposinf(a), 1, np.where(np.isneginf(a), 2, 0)))      # noqa: E731


def forward(x, W, b, seg, lay, relu, pad=0, x_shift=0):
    """out and the route: x and out with `pad` NaN floats behind every row (x `x_shift` floats off 16 bytes), 2 * pad behind every W[g]"""
    import torch
    from gnnmp import grouped
    (N, K), G, Dout = x.shape, W.shape[0], W.shape[1 if lay == 0 else 2]
    Wb = torch.full((G, Dout * K + 2 * pad), float("nan"), dtype=torch.float32, device="cuda")
    Wb[:, :Dout * K] = dev(W).view(G, -1)
    obuf, ov = strided(np.full((N, Dout), np.nan, np.float32), Dout + pad)
    grouped.grouped_launch(strided(x, K + pad, x_shift)[1], K + pad, Wb, Dout * K + 2 * pad, K if lay == 0 else Dout, lay, dev(b),
                           Dout if b is not None and b.ndim == 2 else 0, dev(seg), relu, ov, Dout + pad, N, G, K, Dout)
    out = ov.cpu().numpy()
    ov.fill_(float("nan"))
    assert torch.isnan(obuf).all(), "something was written between or around the rows of out"
    return out, grouped.last_route()


def reached(why, route, sizes, Dout):
    """the property the case exists for, from [kernel, ncb, waves, grid.x] of the launch"""
    from gnnmp import grouped
    kernel, ncb, waves, grid_x = route
    N, cb = sum(sizes), (Dout + 15) // 16
    if why == "multiwave":
        assert kernel == grouped.ROUTE_T16 and waves >= 2 and GC.check_cut(sizes, waves), route
    elif why in ("ncb4", "ncb6"):
        assert kernel == grouped.ROUTE_T16 and ncb == int(why[3]), route
    elif why == "stepdown":
        assert kernel == grouped.ROUTE_T16 and ncb < (8 if cb >= 8 else 7 if cb == 7 else 6 if cb > 4 else 4 if cb > 2 else 2), route
        assert -(-Dout // (ncb * 16)) > 1, "the step-down left one column tile"
    elif why == "fma_aligned":
        assert kernel == grouped.ROUTE_FMA, route
    elif why in ("persistent", "persistent_multiwave"):
        assert kernel == grouped.ROUTE_T16 and grid_x * waves * 16 < N and (why == "persistent" or waves >= 2), route
    else:
        assert why == "fma_multiblock" and kernel == grouped.ROUTE_FMA and grid_x > 1, route


@pytest.mark.parametrize("case", GC.GEOM_FWD, ids=[c[0] for c in GC.GEOM_FWD])
def test_forward_geometry_against_float64(case):
    name, sizes, K, Dout, lay, bias, relu, pad, x_shift, why, _ = case
    sizes = sizes() if callable(sizes) else sizes
    seg, N, G = GC.seg_of(sizes), sum(sizes), len(sizes)
    for kind in ("gauss", "int"):
        rng = np.random.default_rng(K * 1000 + Dout)
        x, W = draw(rng, kind, N, K), draw(rng, kind, G, *((Dout, K) if lay == 0 else (K, Dout)))
        b = None if bias is None else draw(rng, kind, *((G, Dout) if bias == "group" else (Dout,)))
        got, route = forward(x, W, b, seg, lay, relu, pad, x_shift)
        reached(why, route, sizes, Dout)
        bound = (K + 2) * U * GC.forward64(np.abs(x), np.abs(W), seg, None if b is None else np.abs(b), 0, lay)
        err = np.abs(got - GC.forward64(x, W, seg, b, relu, lay))
        print(f"{name} {kind}: route {route}, {int((err > 0).sum())} of {err.size} elements off, worst {err.max():.3e}, "
              f"worst share of the bound {np.max(err / np.maximum(bound, 1e-300)):.3f}")
        assert np.all(err <= (bound if kind == "gauss" else 0.0)), f"{kind}: {int((err > 0).sum())} elements off, worst {err.max():.3e}"
        assert np.array_equal(bits(forward(x, W, b, seg, lay, relu, pad, x_shift)[0]), bits(got)), "two calls differ in bits"


def grad(dz, x, seg, K, Dout, want_w, db_mode, pad=0, shift=0, workspace=False):
    """(dW [G, Dout, K] | None, db | None, route[, the partials]) of one call: NaN padding behind the rows of dz and x and behind every dW[g]"""
    import torch
    from gnnmp import _lib as L, grouped
    G, N = len(seg) - 1, dz.shape[0]
    dW = torch.full((G, Dout * K + pad), float("nan"), device="cuda") if want_w else None
    db = None if db_mode is None else torch.full((G, Dout) if db_mode == "group" else (Dout,), float("nan"), device="cuda")
    dzv, xv, sp = strided(dz, Dout + pad, shift)[1], strided(x, K + pad, shift)[1] if want_w else None, dev(seg)
    if not workspace:
        grouped.grouped_grad_launch(dzv, Dout + pad, xv, K + pad, sp, dW, Dout * K + pad, db, Dout if db_mode == "group" else 0, N, G, K, Dout)
        ws = None
    else:       # the same call with the workspace kept, to look at the slabs' partials
        lib = L.load()
        ws = torch.full((max(1, lib.gnnmp_grouped_dense_grad_workspace(N, G, Dout, K)),), float("nan"), device="cuda")
        job = L.GroupedDenseGradJob(L.ptr(dzv), Dout + pad, L.ptr(xv), K + pad, L.ptr(sp), L.ptr(dW), Dout * K + pad, L.ptr(db),
                                    Dout if db_mode == "group" else 0, L.ptr(ws), ws.numel())
        L.check(lib.gnnmp_grouped_dense_grad_w_f32(ctypes.byref(job), N, G, K, Dout, L.stream_ptr()))
    assert dW is None or pad == 0 or torch.isnan(dW[:, Dout * K:]).all(), "something was written behind a dW[g]"
    res = (None if dW is None else dW[:, :Dout * K].reshape(G, Dout, K).cpu().numpy(), None if db is None else db.cpu().numpy(), grouped.last_route())
    return res + (ws.cpu().numpy(),) if workspace else res


@pytest.mark.parametrize("case", GC.GEOM_GRAD, ids=[c[0] for c in GC.GEOM_GRAD])
def test_weight_gradient_geometry_against_float64(case):
    name, sizes, K, Dout, want_w, db_mode, pad, shift, slabs, at256 = case
    seg, N, G, rows = GC.seg_of(sizes), sum(sizes), len(sizes), np.array(sizes, np.float64)
    for kind in ("gauss", "int"):
        rng = np.random.default_rng(K * 1000 + Dout + 1)
        dz, x = draw(rng, kind, N, Dout), draw(rng, kind, N, K)
        dW, db, (kernel, S, waves, grid_x) = grad(dz, x, seg, K, Dout, want_w, db_mode, pad, shift)
        # the kernel and the waves of its block follow from the shape alone; S and with it grid.x from the CU count too
        assert (kernel, waves) == (at256[0], at256[2]) and S >= slabs and grid_x == G * S, (kernel, S, waves, grid_x)
        (rW, rb), (mW, mb) = GC.grad64(dz, x, seg, db_mode == "shared"), GC.grad64(np.abs(dz), np.abs(x), seg, db_mode == "shared")
        bW, bb = (rows + S)[:, None, None] * U * mW, ((rows + S)[:, None] if db_mode == "group" else N + G * S) * U * mb
        for what, got, ref, bound in (("dW", dW, rW, bW), ("db", db, rb, bb)):
            if got is None:
                continue
            err = np.abs(got - ref)
            print(f"{name} {kind} {what}: S {S}, {int((err > 0).sum())} of {err.size} elements off, worst {err.max():.3e}, "
                  f"worst share of the bound {np.max(err / np.maximum(bound, 1e-300)):.3f}")
            assert np.all(err <= (bound if kind == "gauss" else 0.0)), (kind, what)
        assert dW is None or not dW[rows == 0].any(), "an empty group's gradient is zeros, written"
        assert db is None or db_mode == "shared" or not db[rows == 0].any(), "an empty group's gradient is zeros, written"
        again = grad(dz, x, seg, K, Dout, want_w, db_mode, pad, shift)
        assert all(a is None or np.array_equal(bits(a), bits(b)) for a, b in zip(again[:2], (dW, db))), "two calls differ in bits"


@pytest.mark.parametrize("K,Dout,pad", [(20, 12, 4), (5, 7, 1)], ids=["mfma", "fma"])
def test_slabs_are_runs_of_a_multiple_of_four_rows(K, Dout, pad):
    """grouped_slab's cut, looked at in the workspace: slab s of a group of n rows is rows [s r, (s + 1) r) of it with
    r = ceil(n / S) rounded up to 4 — the four rows of an MFMA step never straddle slabs —, so a group of fewer than 4 S rows leaves
    slabs without rows, and their partials are zeros, written (the fold adds all S)."""
    from gnnmp import grouped
    sizes = GC.SLABS4
    seg, N, G = GC.seg_of(sizes), sum(sizes), len(sizes)
    rng = np.random.default_rng(K + Dout)
    dz, x = draw(rng, "int", N, Dout), draw(rng, "int", N, K)
    dW, db, (kernel, S, _, _), ws = grad(dz, x, seg, K, Dout, True, "group", pad, 0, workspace=True)
    assert kernel == (grouped.ROUTE_GRADW16 if K % 4 == 0 else grouped.ROUTE_GRADW_FMA) and S >= 3 and ws.size == G * S * (Dout * K + Dout)
    part_w, part_b = ws[:G * S * Dout * K].reshape(G, S, Dout, K), ws[G * S * Dout * K:].reshape(G, S, Dout)
    empty = 0
    for g in range(G):
        r = (-(-sizes[g] // S) + 3) & ~3
        for s in range(S):
            n0 = min(seg[g + 1], seg[g] + s * r)
            n1 = min(seg[g + 1], n0 + r)
            empty += n0 == n1
            assert np.array_equal(part_w[g, s], dz[n0:n1].astype(np.float64).T @ x[n0:n1]), (g, s)
            assert np.array_equal(part_b[g, s], dz[n0:n1].astype(np.float64).sum(0)), (g, s)
    assert empty >= S + 4, "the case has an empty group and four groups shorter than 4 S rows"
    assert np.array_equal(dW, part_w.astype(np.float64).sum(1)) and np.array_equal(db, part_b.astype(np.float64).sum(1))


@pytest.mark.parametrize("K,Dout,pad,want", [(20, 12, 4, "T16"), (5, 7, 1, "FMA")], ids=["t16", "fma"])
def test_forward_non_finite_values_stay_in_their_group(K, Dout, pad, want):
    """NaN in rows of x, +Inf in W[g] and bias[g] of one group whose rows share a 16-row tile with both neighbours: every other group's
    rows keep the bits of the finite run (a masked row is a select, never a product), the group's own rows have float64's class element
    by element, and under relu a NaN stays a NaN (NNlib's ifelse(x < 0, 0, x)) on both routes."""
    from gnnmp import grouped
    sizes, gp = GC.CUT, GC.CUT_POISON
    seg, N, G = GC.seg_of(sizes), sum(sizes), len(sizes)
    lo, hi = int(seg[gp]), int(seg[gp + 1])
    assert hi - lo >= 5 and lo // 16 == (hi - 1) // 16 == (lo - 1) // 16 and any(seg[g + 1] > hi and seg[g] // 16 == lo // 16 for g in range(gp + 1, G))
    rng = np.random.default_rng(K + Dout)
    x, W, b = draw(rng, "gauss", N, K), draw(rng, "gauss", G, Dout, K), draw(rng, "gauss", G, Dout)
    px, pW, pb = x.copy(), W.copy(), b.copy()
    px[lo + 1, 1:3], px[lo + 3, 0] = NAN, NAN                 # rows lo, lo + 2, lo + 4 stay finite
    pW[gp, 0, 1], pW[gp, 3, 0], pW[gp, 3, 2], pb[gp, 1] = INF, INF, INF, INF
    others = np.ones(N, bool)
    others[lo:hi] = False
    for relu in (0, 1):
        clean, route = forward(x, W, b, seg, 0, relu, pad)
        assert route[0] == getattr(grouped, "ROUTE_" + want) and (want == "FMA" or (route[2] >= 2 and GC.check_cut(sizes, route[2]))), route
        got = forward(px, pW, pb, seg, 0, relu, pad)[0]
        assert np.array_equal(bits(got[others]), bits(clean[others])), "a non-finite value of one group reached another group's rows"
        with np.errstate(invalid="ignore"):
            ref = GC.forward64(px, pW, seg, pb, relu, 0)[lo:hi]
            bound = (K + 2) * U * GC.forward64(np.abs(x), np.abs(W), seg, np.abs(b), 0, 0)[lo:hi]
        kg, kr = klass(got[lo:hi]), klass(ref)
        assert np.array_equal(kg, kr), f"classes differ at {np.argwhere(kg != kr).tolist()}"
        fin = kr == 0
        assert np.all(np.abs(got[lo:hi][fin] - ref[fin]) <= bound[fin])
        # what the poison must have produced for the check to mean something: all four classes without relu; with it NaN stays, -Inf is 0
        assert set(np.unique(kr)) == ({0, 1, 2, 3} if not relu else {0, 1, 3}) and np.isnan(got[lo + 1]).all()


@pytest.mark.parametrize("K,Dout,pad", [(20, 12, 4), (5, 7, 1)], ids=["mfma", "fma"])
def test_gradient_non_finite_values_stay_in_their_group(K, Dout, pad):
    """NaN and ±Inf in the rows of dz and x of one short group between two others: every other group's dW and db keep the bits of the
    finite run, the group's own have float64's class element by element.  Then dz = +Inf in the LAST row of every group, x finite and
    non-zero: dW is ±Inf where float64 says so and nowhere NaN — the rows behind a slab's end re-read its last row, and a pad row that
    was multiplied by zero instead of replaced would give 0 * Inf."""
    from gnnmp import grouped
    sizes, gp = GC.SLABS4, GC.SLABS4_POISON
    seg, N, G, rows = GC.seg_of(sizes), sum(sizes), len(sizes), np.array(sizes)
    lo, hi = int(seg[gp]), int(seg[gp + 1])
    assert hi - lo == 5 and sizes[gp - 1] and sizes[gp + 1]
    rng = np.random.default_rng(K + Dout + 1)
    dz, x = draw(rng, "gauss", N, Dout), draw(rng, "gauss", N, K)
    cW, cb, (kernel, S, _, _) = grad(dz, x, seg, K, Dout, True, "group", pad)
    assert kernel == (grouped.ROUTE_GRADW16 if K % 4 == 0 else grouped.ROUTE_GRADW_FMA) and S >= 3
    pdz, px = dz.copy(), x.copy()
    pdz[lo, 0], pdz[lo + 2, 2], pdz[hi - 1, 1] = NAN, INF, -INF      # row hi - 1 is alone in its slab: three pad rows behind it
    px[lo + 1, 1], px[lo + 3, 3] = INF, NAN
    gW, gb, _ = grad(pdz, px, seg, K, Dout, True, "group", pad)
    others = np.arange(G) != gp
    assert np.array_equal(bits(gW[others]), bits(cW[others])) and np.array_equal(bits(gb[others]), bits(cb[others])), \
        "a non-finite value of one group reached another group's gradient"
    with np.errstate(invalid="ignore"):
        rW, rb = GC.grad64(pdz, px, seg)
    assert np.array_equal(klass(gW[gp]), klass(rW[gp])) and np.array_equal(klass(gb[gp]), klass(rb[gp]))
    assert set(np.unique(klass(rW[gp]))) == {0, 1, 2, 3}
    # +Inf in the last row of every group
    last = seg[1:][rows > 0] - 1
    pdz = dz.copy()
    pdz[last] = INF
    gW, gb, _ = grad(pdz, x, seg, K, Dout, True, "group", pad)
    with np.errstate(invalid="ignore"):
        rW, rb = GC.grad64(pdz, x, seg)
    assert not np.isnan(rW).any() and not np.isnan(gW).any(), f"{int(np.isnan(gW).sum())} NaN in dW"
    assert np.array_equal(klass(gW), klass(rW)) and np.array_equal(klass(gb), klass(rb))
    assert np.isinf(gW[rows > 0]).all() and np.isposinf(gb[rows > 0]).all() and not gW[rows == 0].any() and not gb[rows == 0].any()
