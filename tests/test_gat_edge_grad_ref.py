"""tests/gat_edge_grad_ref.py on trial (CPU): every gradient of the float64 restatement against central differences on a bipartite
relation with multi-edges (n_src = 5, n_dst = 9, E = 40, H = 3, C = 2, ein = 3), the square relation and the whole layer the same way,
and its forward against the oracle's gat_conv_edge.

The bound of the differences is a relative error of 1e-6: the formulas are on trial, not the arithmetic — float64 central differences
with step 1e-6 agree with a right formula to about 3e-9 here (truncation h^2 f''' / 6 ~ 1e-12, rounding eps / h ~ 2e-10 of the loss's
scale), a wrong term is off by O(1).  The forward's bound against the float32 oracle is that of tests/test_gat_edge_features.py, 5e-6
norm-wise."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gat_edge_grad_ref as R  # noqa: E402

BOUND = 1e-6
STEP = 1e-6
N_SRC, N_DST, E, H, C, EIN, SLOPE = 5, 9, 40, 3, 2, 3, 0.2


def _relation(seed, n_src, n_dst):
    rng = np.random.default_rng(seed)
    s, t = rng.integers(0, n_src, E), rng.integers(0, n_dst - 1, E)      # the last destination has no in-edge
    s[1], t[1] = s[0], t[0]                                               # a pair listed twice (with another e below)
    s[7], t[7] = s[3], t[3]
    return rng, s, t


def _numeric(f, v):
    """central differences of the scalar f at the array v"""
    g = np.zeros_like(v)
    it = np.nditer(v, flags=["multi_index"])
    for _ in it:
        i = it.multi_index
        keep = v[i]
        v[i] = keep + STEP
        up = f()
        v[i] = keep - STEP
        dn = f()
        v[i] = keep
        g[i] = (up - dn) / (2 * STEP)
    return g


def _rel(got, want):
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-300))


def test_the_relation_has_multi_edges_and_an_empty_row():
    _, s, t = _relation(0, N_SRC, N_DST)
    pairs = s * N_DST + t
    assert len(np.unique(pairs)) < E and (np.bincount(t, minlength=N_DST) == 0).any()
    assert (np.bincount(pairs).max() >= 2)


def test_bipartite_gradients_against_central_differences():
    rng, s, t = _relation(0, N_SRC, N_DST)
    Ws, Wd = rng.standard_normal((N_SRC, H, C)), rng.standard_normal((N_DST, H, C))
    a, a_e = rng.standard_normal((H, 2 * C)), rng.standard_normal((H, C))
    e, We = rng.standard_normal((E, EIN)), rng.standard_normal((H * C, EIN))
    do = rng.standard_normal((N_DST, H, C))

    def loss():
        es = e @ R.fold(a_e, We).T
        return float((do * R.core(s, t, N_SRC, N_DST, Ws, Wd, a, es, SLOPE)[0]).sum())

    M = R.fold(a_e, We)
    es = e @ M.T
    o, c = R.core(s, t, N_SRC, N_DST, Ws, Wd, a, es, SLOPE)
    assert np.all(o[N_DST - 1] == 0) and np.all(c["den"][N_DST - 1] == 0)
    gr = R.core_grad(s, t, N_SRC, N_DST, Ws, Wd, a, es, SLOPE, c, do)
    dM = gr["des"].T @ e
    dWe, da_e = R.fold_grad(a_e, We, dM)
    got = dict(Wx_src=gr["dWx_src"], Wx_dst=gr["dWx_dst"], a=gr["da"], e=gr["des"] @ M, W_e=dWe, a_e=da_e)
    var = dict(Wx_src=Ws, Wx_dst=Wd, a=a, e=e, W_e=We, a_e=a_e)
    worst = {k: _rel(got[k], _numeric(loss, var[k])) for k in var}
    print("relative error of each gradient against central differences:", worst)
    assert max(worst.values()) <= BOUND, worst
    # des itself: the gradient with respect to an es that is a free variable
    es_free = es.copy()
    lf = lambda: float((do * R.core(s, t, N_SRC, N_DST, Ws, Wd, a, es_free, SLOPE)[0]).sum())      # noqa: E731
    assert _rel(gr["des"], _numeric(lf, es_free)) <= BOUND
    assert np.allclose(gr["dsd"], R.seg_sum(t, gr["des"], N_DST)) and np.allclose(gr["dss"], R.seg_sum(s, gr["des"], N_SRC))


def test_square_gradients_fold_the_target_term_into_the_source_rows():
    n = 7
    rng, s, t = _relation(1, n, n)
    Wx, a, es, do = rng.standard_normal((n, H, C)), rng.standard_normal((H, 2 * C)), rng.standard_normal((E, H)), rng.standard_normal((n, H, C))
    loss = lambda: float((do * R.core(s, t, n, n, Wx, None, a, es, SLOPE)[0]).sum())      # noqa: E731
    o, c = R.core(s, t, n, n, Wx, None, a, es, SLOPE)
    gr = R.core_grad(s, t, n, n, Wx, None, a, es, SLOPE, c, do)
    assert gr["dWx_dst"] is None
    worst = {"Wx": _rel(gr["dWx_src"], _numeric(loss, Wx)), "a": _rel(gr["da"], _numeric(loss, a)), "es": _rel(gr["des"], _numeric(loss, es))}
    assert max(worst.values()) <= BOUND, worst
    # the same relation with Wx_dst given as a copy: the two halves add up to the folded gradient
    split = R.core_grad(s, t, n, n, Wx, Wx.copy(), a, es, SLOPE, c, do)
    assert np.allclose(split["dWx_src"] + split["dWx_dst"], gr["dWx_src"], rtol=0, atol=1e-13)


def test_layer_gradients_against_central_differences():
    n, Din = 8, 4
    for concat, sigma, with_b in ((True, "relu", True), (False, None, True), (True, None, False)):
        rng, s, t = _relation(2 + int(concat), n, n)
        x, e = rng.standard_normal((n, Din)), rng.standard_normal((E, EIN))
        W, We, a = rng.standard_normal((H * C, Din)), rng.standard_normal((H * C, EIN)), rng.standard_normal((3 * C, H))
        b = rng.standard_normal(H * C if concat else C) if with_b else None
        dy = rng.standard_normal((n, H * C if concat else C))
        args = lambda: (s, t, n, x, e, W, We, a, b, sigma, H, concat)      # noqa: E731
        loss = lambda: float((dy * R.layer(*args())[0]).sum())             # noqa: E731
        y, c = R.layer(*args())
        gr = R.layer_grad(*args(), c, dy)
        var = dict(dx=x, de=e, dW=W, dWe=We, da=a, **({"db": b} if with_b else {}))
        worst = {k: _rel(gr[k], _numeric(loss, v)) for k, v in var.items()}
        assert max(worst.values()) <= BOUND, (concat, sigma, worst)
        assert gr["db"] is None or with_b


def test_forward_against_the_oracle(oracle):
    from oracle import attn_layers as AL
    n, Din = 40, 5
    rng = np.random.default_rng(5)
    s, t = rng.integers(1, n + 1, 300), rng.integers(1, n - 3, 300)
    s[1], t[1] = s[0], t[0]
    f32 = np.float32
    x, e = rng.standard_normal((n, Din)).astype(f32), rng.standard_normal((300, EIN)).astype(f32)
    W = (rng.standard_normal((H * C, Din)) / np.sqrt(Din)).astype(f32)
    We = (rng.standard_normal((H * C, EIN)) / np.sqrt(EIN)).astype(f32)
    a = (rng.standard_normal((3 * C, H)) * 0.6).astype(f32)
    for concat in (True, False):
        b = (rng.standard_normal(H * C if concat else C) * 0.1).astype(f32)
        want = AL.gat_conv_edge(s, t, n, x, e, W, We, a, b, "relu", heads=H, concat=concat)
        got, _ = R.layer(s - 1, t - 1, n, x, e, W, We, a, b, "relu", H, concat)
        assert got.shape == want.shape
        assert np.linalg.norm(got - want) <= 5e-6 * np.linalg.norm(want)
