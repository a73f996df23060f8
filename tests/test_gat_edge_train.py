"""Training GATConv with edge features: gat_conv_ad(l, g, x, e) (gnnmp/backward.py: _GATConvEdgeFn) against the float64 restatement
tests/gat_edge_grad_ref.py (pinned by tests/test_gat_edge_grad_ref.py), at the four (H, C, Din, ein, concat) rows of
tests/test_gat_edge_features.py.

One graph of 300 nodes and 3000 shuffled edges (plan slot != edge position): a hub row of 700 in-edges, which both plans chunk, a row
whose only in-edge is known, rows without in-edges.  Every gradient — x, e, dense_x, dense_e, all three thirds of a, bias — owes 1e-5 of
the reference, norm-wise and element-wise against the array's scale (the project's bar for every adjoint).  Then: W_e = 0 against the
e-less adjoint; the one-edge row's de; equal bits of two calls; the refusals; three SGD steps on a 2-layer model."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gat_edge_grad_ref as R  # noqa: E402

gpu = pytest.mark.gpu
ROWS = [(8, 16, 100, 12, True), (4, 8, 20, 3, False), (1, 7, 9, 5, True), (2, 4, 6, 1, True)]      # tests/test_gat_edge_features.py
N, E, HUB, HUB_DEG, LONE = 300, 3000, 9, 700, 294
BOUND = 1e-5
f32 = np.float32


@functools.lru_cache(maxsize=None)
def _graph():
    """0-based (s, t, k_lone): t[k_lone] = LONE is that row's only edge; rows 295 .. 299 have no in-edge"""
    rng = np.random.default_rng(11)
    s, t = rng.integers(0, N, E), rng.integers(0, LONE, E)
    t[:HUB_DEG] = HUB
    t[HUB_DEG] = LONE
    p = rng.permutation(E)
    s, t = s[p], t[p]
    (k_lone,) = np.flatnonzero(t == LONE)
    return s, t, int(k_lone)


@functools.lru_cache(maxsize=None)
def _problem(H, C, Din, ein, concat):
    """inputs, parameters, the upstream gradient and the float64 reference of one row; computed once, shared, left unchanged"""
    rng = np.random.default_rng(1000 * H + 10 * C + ein)
    s, t, _ = _graph()
    sigma = "relu" if H in (8, 1) else None
    p = dict(x=rng.standard_normal((N, Din)), e=rng.standard_normal((E, ein)), W=rng.standard_normal((H * C, Din)) / np.sqrt(Din),
             We=rng.standard_normal((H * C, ein)) / np.sqrt(ein), a=rng.standard_normal((3 * C, H)) * 0.6,
             b=rng.standard_normal(H * C if concat else C) * 0.1, dy=rng.standard_normal((N, H * C if concat else C)))
    p = {k: v.astype(f32) for k, v in p.items()}
    y, c = R.layer(s, t, N, p["x"], p["e"], p["W"], p["We"], p["a"], p["b"], sigma, H, concat)
    gr = R.layer_grad(s, t, N, p["x"], p["e"], p["W"], p["We"], p["a"], p["b"], sigma, H, concat, c, p["dy"])
    for v in p.values():
        v.setflags(write=False)
    return p, sigma, y, gr


def _dev(v, grad=False):
    import torch
    return torch.from_numpy(np.array(v)).cuda().requires_grad_(grad)      # (a copy: the shared problem stays read-only)


def _gnn_graph():
    import gnnmp
    s, t, _ = _graph()
    return gnnmp.GNNGraph(_dev(s + 1), _dev(t + 1), num_nodes=N)


def _layer(p, sigma, H, C, Din, ein, concat, grad=True, edge=True):
    import gnnmp
    l = gnnmp.GATConv(((Din, ein), C) if edge else (Din, C), sigma, heads=H, concat=concat, add_self_loops=False, seed=1)
    l.dense_x_weight, l.bias = _dev(p["W"], grad), _dev(p["b"], grad)
    if edge:
        l.dense_e_weight, l.a = _dev(p["We"], grad), _dev(p["a"], grad)
    else:
        l.a = _dev(p["a"][:2 * C], grad)
    return l


def _run(p, sigma, H, C, Din, ein, concat):
    """(y, {name: gradient}) of one gat_conv_ad call and its backward, as numpy"""
    from gnnmp.backward import gat_conv_ad
    g = _gnn_graph()
    l = _layer(p, sigma, H, C, Din, ein, concat)
    x, e = _dev(p["x"], True), _dev(p["e"], True)
    y = gat_conv_ad(l, g, x, e)
    y.backward(_dev(p["dy"]))
    got = dict(dx=x.grad, de=e.grad, dW=l.dense_x_weight.grad, dWe=l.dense_e_weight.grad, da=l.a.grad, db=l.bias.grad)
    return y.detach().cpu().numpy(), {k: v.cpu().numpy() for k, v in got.items()}


def _close(got, ref, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, what
    nrm = np.linalg.norm(got - ref) / np.linalg.norm(ref)
    worst = np.abs(got - ref).max() / np.abs(ref).max()
    print(f"{what}: {nrm:.2e} norm-wise, {worst:.2e} of the array's scale")
    return nrm <= BOUND and worst <= BOUND


@gpu
@pytest.mark.parametrize("H,C,Din,ein,concat", ROWS)
def test_every_gradient_against_float64(H, C, Din, ein, concat):
    p, sigma, y_ref, gr = _problem(H, C, Din, ein, concat)
    y, got = _run(p, sigma, H, C, Din, ein, concat)
    bad = [] if _close(y, y_ref, "y") else ["y"]
    bad += [k for k in ("dx", "de", "dW", "dWe", "da", "db") if not _close(got[k], gr[k], k)]
    assert not bad, bad
    C3 = got["da"].reshape(3, C, H)                      # all three thirds of a carry a gradient: target, source and edge
    assert all(np.abs(C3[k]).max() > 0 for k in range(3))


@gpu
def test_zero_edge_weights_agree_with_the_e_less_adjoint():
    """W_e = 0: es = 0, the layer is the e-less GATConv — another forward and another pullback kernel (the o+ / P shortcut), so the x, weight
    and a[:2C] gradients agree within the bound, not bit for bit; and nothing flows into e"""
    from gnnmp.backward import gat_conv_ad
    H, C, Din, ein, concat = ROWS[1]
    p, sigma, _, _ = _problem(H, C, Din, ein, concat)
    p = dict(p, We=np.zeros_like(p["We"]))
    g = _gnn_graph()
    l, l0 = _layer(p, sigma, H, C, Din, ein, concat), _layer(p, sigma, H, C, Din, ein, concat, edge=False)
    x, x0, e = _dev(p["x"], True), _dev(p["x"], True), _dev(p["e"], True)
    y, y0 = gat_conv_ad(l, g, x, e), gat_conv_ad(l0, g, x0)
    y.backward(_dev(p["dy"]))
    y0.backward(_dev(p["dy"]))
    n = lambda v: v.detach().cpu().numpy()      # noqa: E731
    ok = [_close(n(y), n(y0), "y"), _close(n(x.grad), n(x0.grad), "dx"), _close(n(l.dense_x_weight.grad), n(l0.dense_x_weight.grad), "dW"),
          _close(n(l.a.grad)[:2 * C], n(l0.a.grad), "da[:2C]"), _close(n(l.bias.grad), n(l0.bias.grad), "db")]
    assert all(ok), ok
    assert not n(e.grad).any()                           # de = des M with M = 0


@gpu
def test_the_only_edge_of_a_row_gets_no_gradient():
    """a row with one in-edge has α = 1 whatever the logit: dz = α (g - D) cancels, so de_k owes at most 1e-5 of the largest |de|"""
    H, C, Din, ein, concat = ROWS[0]
    p, sigma, _, gr = _problem(H, C, Din, ein, concat)
    _, got = _run(p, sigma, H, C, Din, ein, concat)
    k = _graph()[2]
    assert np.abs(gr["de"][k]).max() <= 1e-12 * np.abs(gr["de"]).max()
    assert np.abs(got["de"][k]).max() <= BOUND * np.abs(got["de"]).max()


@gpu
def test_two_calls_give_equal_bits():
    H, C, Din, ein, concat = ROWS[3]
    p, sigma, _, _ = _problem(H, C, Din, ein, concat)
    y1, g1 = _run(p, sigma, H, C, Din, ein, concat)
    y2, g2 = _run(p, sigma, H, C, Din, ein, concat)
    assert np.array_equal(y1, y2) and all(np.array_equal(g1[k], g2[k]) for k in g1)


@gpu
def test_needs_input_grad_prunes_and_refusals():
    import torch
    import gnnmp
    from gnnmp.backward import gat_conv_ad
    H, C, Din, ein, concat = ROWS[3]
    p, sigma, _, gr = _problem(H, C, Din, ein, concat)
    g = _gnn_graph()
    # only e asks for a gradient: the same de, nothing else
    l = _layer(p, sigma, H, C, Din, ein, concat, grad=False)
    x, e = _dev(p["x"]), _dev(p["e"], True)
    gat_conv_ad(l, g, x, e).backward(_dev(p["dy"]))
    assert _close(e.grad.cpu().numpy(), gr["de"], "de alone") and x.grad is None and l.a.grad is None and l.dense_e_weight.grad is None
    # the reference's assertions on e (conv.jl:114-121), a wrong edge count, and the positional seed of the old signature
    with pytest.raises(AssertionError, match="Input edge features required"):
        gat_conv_ad(l, g, x)
    l0 = _layer(p, sigma, H, C, Din, ein, concat, grad=False, edge=False)
    with pytest.raises(AssertionError, match="not specified in the layer constructor"):
        gat_conv_ad(l0, g, x, e)
    with pytest.raises(AssertionError):
        gat_conv_ad(l, g, x, _dev(p["e"][:-1]))
    with pytest.raises(TypeError, match="seed="):
        gat_conv_ad(l0, g, x, 1234)
    ld = gnnmp.GATConv((Din, C), heads=H, add_self_loops=False, dropout=0.5, seed=1)
    y1, y2 = gat_conv_ad(ld, g, x, seed=7), gat_conv_ad(ld, g, x, None, 7)      # e = None, seed by keyword or in its new place
    assert torch.equal(y1, y2) and ld.last_seed == 7


@gpu
def test_three_sgd_steps_lower_the_loss():
    """a 2-layer model, both layers with edge features, every parameter and nothing else updated: plain gradient descent on a
    mean-squared error goes down step by step"""
    import torch
    import gnnmp
    from gnnmp.backward import gat_conv_ad
    rng = np.random.default_rng(3)
    Din, ein = 6, 3
    g = _gnn_graph()
    x, e = _dev(rng.standard_normal((N, Din)).astype(f32)), _dev(rng.standard_normal((E, ein)).astype(f32))
    target = _dev(rng.standard_normal((N, 4)).astype(f32))
    l1 = gnnmp.GATConv(((Din, ein), 8), "relu", heads=2, add_self_loops=False, seed=5)
    l2 = gnnmp.GATConv(((16, ein), 4), None, heads=3, concat=False, add_self_loops=False, seed=6)
    params = []
    for l in (l1, l2):
        for name in ("dense_x_weight", "dense_e_weight", "a", "bias"):
            setattr(l, name, getattr(l, name).detach().clone().requires_grad_(True))
            params.append(getattr(l, name))
    losses = []
    for _ in range(4):
        loss = ((gat_conv_ad(l2, g, gat_conv_ad(l1, g, x, e), e) - target) ** 2).mean()
        losses.append(float(loss.detach()))
        for q in params:
            q.grad = None
        loss.backward()
        assert all(q.grad is not None and torch.isfinite(q.grad).all() for q in params)
        with torch.no_grad():
            for q in params:
                q -= 0.05 * q.grad
    print("losses:", losses)
    assert losses[1] < losses[0] and losses[2] < losses[1] and losses[3] < losses[2]
