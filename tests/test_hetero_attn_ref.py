"""tests/hetero_attn_ref.py pinned without a GPU: on a relation whose source and destination type coincide, with x_src = x_dst, its layer
forwards reproduce oracle.gat_conv and oracle/attn_layers.gatv2_conv (add_self_loops off); its gradients agree with central differences
in float64 on a bipartite relation and through a whole HeteroGraphConv (fold +, max and min; σ identity and relu; concat on and off)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hetero_attn_ref as R  # noqa: E402

H_STEP, TOL = 1e-6, 1e-6


def _layer(rng, kind, cin, H, C, sigma, concat, bias=True):
    nb = H * C if concat else C
    b = rng.uniform(-1, 1, nb) if bias else None
    if kind == R.GAT:
        return R.gat_params(rng.uniform(-1, 1, (H * C, cin)), rng.uniform(-1, 1, (2 * C, H)), b, H, sigma, concat)
    return R.gatv2_params(rng.uniform(-1, 1, (H * C, cin)), rng.uniform(-1, 1, H * C) if bias else None, rng.uniform(-1, 1, (H * C, cin)),
                          rng.uniform(-1, 1, (C, H)), b, H, sigma, concat)


@pytest.mark.parametrize("concat", [True, False])
@pytest.mark.parametrize("sigma", [None, "relu"])
def test_square_relation_reproduces_the_oracles(sigma, concat):
    from oracle import attn_layers as AL
    from oracle import oracle as O
    O.build()
    rng = np.random.default_rng(7)
    n, E, cin, H, C = 12, 40, 5, 3, 4
    s, t = rng.integers(0, n, E), rng.integers(0, n, E)
    x = rng.uniform(-1, 1, (n, cin)).astype(np.float32)
    f = lambda v: None if v is None else np.asarray(v, np.float32)      # noqa: E731
    p = _layer(rng, R.GAT, cin, H, C, sigma, concat)
    p = {k: (f(v).astype(np.float64) if isinstance(v, np.ndarray) else v) for k, v in p.items()}
    want = O.gat_conv(s + 1, t + 1, n, x, f(p["W"]), f(p["a"]), f(p["bias"]), sigma, H, concat, 0.2, add_self_loops_=False)
    got = R.layer_forward(p, s, t, n, x, x)
    assert np.abs(got - want).max() <= 1e-5 * max(np.abs(want).max(), 1.0)
    p = _layer(rng, R.GATV2, cin, H, C, sigma, concat)
    p = {k: (f(v).astype(np.float64) if isinstance(v, np.ndarray) else v) for k, v in p.items()}
    want = AL.gatv2_conv(s + 1, t + 1, n, x, f(p["Wi"]), f(p["bi"]), f(p["Wj"]), f(p["a"]), f(p["bias"]), sigma, H, concat, 0.2, add_self_loops_=False)
    got = R.layer_forward(p, s, t, n, x, x)
    assert np.abs(got - want).max() <= 1e-5 * max(np.abs(want).max(), 1.0)


def _fd(f, arr):
    g = np.zeros_like(arr)
    for i in np.ndindex(arr.shape):
        keep = arr[i]
        arr[i] = keep + H_STEP
        hi = f()
        arr[i] = keep - H_STEP
        lo = f()
        arr[i] = keep
        g[i] = (hi - lo) / (2 * H_STEP)
    return g


def _agree(fd, g, what):
    assert fd.shape == g.shape, what
    assert np.abs(fd - g).max() <= TOL * max(np.abs(g).max(), 1.0), f"{what}: {np.abs(fd - g).max():.3e}"


@pytest.mark.parametrize("concat", [True, False])
@pytest.mark.parametrize("sigma", [None, "relu"])
@pytest.mark.parametrize("kind", [R.GAT, R.GATV2])
def test_layer_gradients_agree_with_central_differences_on_a_bipartite_relation(kind, sigma, concat):
    rng = np.random.default_rng(31 + kind)
    ns, nd, E, cin, H, C = 5, 7, 20, 3, 2, 3
    s, t = rng.integers(0, ns, E), rng.integers(0, nd - 1, E)      # the last destination has no in-edge
    xs, xd = rng.uniform(-1, 1, (ns, cin)), rng.uniform(-1, 1, (nd, cin))
    p = _layer(rng, kind, cin, H, C, sigma, concat)
    dy = rng.uniform(-1, 1, (nd, H * C if concat else C))
    z = R.layer_forward({**p, "sigma": None}, s, t, nd, xs, xd)
    assert np.abs(z).min() > 1e-4 and (z > 0).any() and (z < 0).any(), "a pre-activation too close to relu's kink, or relu never switches"
    f = lambda: float((R.layer_forward(p, s, t, nd, xs, xd) * dy).sum())      # noqa: E731
    dxs, dxd, grads = R.layer_grad(p, s, t, nd, xs, xd, dy)
    _agree(_fd(f, xs), dxs, "Δx_src")
    _agree(_fd(f, xd), dxd, "Δx_dst")
    names = {"W": "W", "a": "a", "bias": "bias"} if kind == R.GAT else {"Wi": "Wi", "bi": "bi", "Wj": "Wj", "a": "a", "bias": "bias"}
    for k in names:
        _agree(_fd(f, p[k]), grads[k], f"Δ{k}")


ETS = [("A", "ab", "B"), ("C", "cb", "B"), ("B", "ba", "A"), ("B", "bb", "B")]      # B is source and destination; C is only a source
NUM = {"A": 5, "B": 6, "C": 4}


@pytest.mark.parametrize("combine,sigma", [("+", None), ("max", "relu"), ("min", None)])
def test_conv_gradients_agree_with_central_differences(combine, sigma):
    rng = np.random.default_rng(23)
    cin, H, C = 3, 2, 2
    coo = {et: (rng.integers(0, NUM[et[0]], 9), rng.integers(0, NUM[et[2]], 9)) for et in ETS}
    x = {k: rng.uniform(-1, 1, (n, cin)) for k, n in NUM.items()}
    members = [(et, _layer(rng, (R.GAT, R.GATV2)[k % 2], cin, H, C, sigma, True)) for k, et in enumerate(ETS)]
    dout = {k: rng.uniform(-1, 1, (NUM[k], H * C)) for k in ("A", "B")}
    if combine != "+":      # no kink within the step: competing terms of the fold apart, unless they tie exactly at relu's zero
        ys = [R.layer_forward(p, *coo[et], NUM["B"], x[et[0]], x["B"]) for et, p in members if et[2] == "B"]
        gaps = np.diff(np.sort(np.stack(ys), axis=0), axis=0)
        assert gaps[gaps > 0].min() > 1e-4

    def f():
        y = R.conv_forward(members, coo, NUM, x, combine)
        return sum(float((y[k] * dout[k]).sum()) for k in y)
    dx, grads = R.conv_grad(members, coo, NUM, x, dout, combine)
    for k in x:
        _agree(_fd(f, x[k]), dx[k], f"Δx[{k}]")
    for (et, p), gr in zip(members, grads):
        for name, gv in gr.items():
            if gv is not None:
                _agree(_fd(f, p[name]), gv, f"Δ{name} {et}")
