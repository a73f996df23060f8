"""Pins tests/attn_edge_ref.py, the float64 reference of GATv2Conv and TransformerConv with edge features, without a GPU:
every analytic gradient against central finite differences of the float64 forward (5 nodes, 9 edges, H = 2, C = 3, ein = 2, h = 1e-6,
1e-6 relative), and the forward against oracle/attn_layers.py when dense_e / W6 is all zeros."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_edge_ref as R  # noqa: E402

N, H, C, EIN, CIN, STEP = 5, 2, 3, 2, 4, 1e-6
S = np.array([0, 1, 2, 3, 4, 0, 2, 1, 1], np.int64)
T = np.array([1, 2, 3, 4, 0, 2, 0, 3, 3], np.int64)      # node 3 has three in-edges, two of them the same pair (1, 3)


def _case(seed, cin=CIN):
    rng = np.random.default_rng(seed)
    return rng, rng.standard_normal((N, cin)), rng.standard_normal((len(S), EIN))


def _fd(loss, arr):
    fd = np.zeros_like(arr)
    for i in np.ndindex(arr.shape):
        keep = arr[i]
        arr[i] = keep + STEP
        hi = loss()
        arr[i] = keep - STEP
        lo = loss()
        arr[i] = keep
        fd[i] = (hi - lo) / (2 * STEP)
    return fd


def _check(loss, operands):
    for what, arr, g in operands:
        fd = _fd(loss, arr)
        err = np.abs(fd - g).max()
        assert err <= 1e-6 * max(np.abs(g).max(), 1.0), (what, err)


@pytest.mark.parametrize("sigma", [None, "relu"])
@pytest.mark.parametrize("concat", [True, False])
def test_gatv2_gradients_agree_with_finite_differences(concat, sigma):
    rng, x, e = _case(11)
    p = {k: (v.astype(np.float64) if isinstance(v, np.ndarray) else v) for k, v in R.gatv2_params(rng, CIN, EIN, H, C, concat, sigma).items()}
    r = rng.standard_normal((N, H * C if concat else C))
    y, c = R.gatv2_layer(S, T, N, x, e, p)
    # the condition on the inputs: no leakyrelu / relu argument within 1000 h of its kink
    assert np.abs(c["extra"][0]).min() > 1e-3 and (sigma is None or np.abs(c["pre"]).min() > 1e-3)
    g = R.gatv2_grad(S, T, N, x, e, p, r)
    loss = lambda: float((R.gatv2_layer(S, T, N, x, e, p)[0] * r).sum())      # noqa: E731
    _check(loss, [("dx", x, g["dx"]), ("de", e, g["de"]), ("dWi", p["Wi"], g["dWi"]), ("dbi", p["bi"], g["dbi"]), ("dWj", p["Wj"], g["dWj"]),
                  ("dWe", p["We"], g["dWe"]), ("da", p["a"], g["da"]), ("dbias", p["bias"], g["dbias"])])


@pytest.mark.parametrize("root,skip", [(True, False), (False, True), (True, True)])
@pytest.mark.parametrize("concat", [True, False])
def test_transformer_gradients_agree_with_finite_differences(concat, root, skip):
    cin = (H * C if concat else C) if skip else CIN
    rng, x, e = _case(12, cin)
    p = {k: (v.astype(np.float64) if isinstance(v, np.ndarray) else v)
         for k, v in R.transformer_params(rng, cin, EIN, H, C, concat, root, skip).items()}
    r = rng.standard_normal((N, H * C if concat else C))
    g = R.transformer_grad(S, T, N, x, e, p, r)
    loss = lambda: float((R.transformer_layer(S, T, N, x, e, p)[0] * r).sum())      # noqa: E731
    ops = [("dx", x, g["dx"]), ("de", e, g["de"])]
    ops += [("d" + k, p[k], g["d" + k]) for k in ("W1", "b1", "W2", "b2", "W3", "b3", "W4", "b4", "W6", "b6") if p[k] is not None]
    _check(loss, ops)


def test_the_attention_core_gradients_agree_with_finite_differences():
    """dQ, dK, dV, dF, da of both cores directly — what the two exports are held to"""
    rng = np.random.default_rng(13)
    Q, K, V = (rng.standard_normal((N, H, C)) for _ in range(3))
    F, a, do = rng.standard_normal((len(S), H, C)), rng.standard_normal((H, C)), rng.standard_normal((N, H, C))
    for mode, scale in (("gatv2", 1.0), ("dot", float(np.sqrt(C)))):
        o, c = R.core(mode, S, T, N, Q, K, V, F, a, 0.2, scale)
        assert mode == "dot" or np.abs(c["extra"][0]).min() > 1e-3
        g = R.core_grad(mode, S, T, N, Q, K, V, F, a, 0.2, scale, c, do)
        loss = lambda: float((R.core(mode, S, T, N, Q, K, V, F, a, 0.2, scale)[0] * do).sum())      # noqa: E731
        ops = [("dQ", Q, g["dQ"]), ("dK", K, g["dK"]), ("dF", F, g["dF"])]
        ops += [("da", a, g["da"])] if mode == "gatv2" else [("dV", V, g["dV"])]
        _check(loss, ops)


@pytest.mark.parametrize("concat", [True, False])
def test_forward_with_zero_edge_weights_is_the_oracle_layer(concat):
    """dense_e = 0 / W6 = 0 (no bias): the edge-featured reference is oracle/attn_layers.py's e-less layer (float32, 1-based) at 1e-5"""
    from oracle import attn_layers as AL
    s, t = R.graph()
    n = R.N_NODES
    rng = np.random.default_rng(14)
    x = rng.standard_normal((n, 8)).astype(np.float32)
    e = rng.standard_normal((len(s), 3)).astype(np.float32)
    p = R.gatv2_params(rng, 8, 3, 2, 6, concat)
    p["We"] = np.zeros_like(p["We"])
    y, _ = R.gatv2_layer(s, t, n, x, e, p)
    ref = AL.gatv2_conv(s + 1, t + 1, n, x, p["Wi"], p["bi"], p["Wj"], p["a"], p["bias"], "relu", heads=2, concat=concat,
                        add_self_loops_=False)
    assert R.rel(ref, y) <= 1e-5
    q = R.transformer_params(rng, 8, 3, 2, 6, concat, True, False)
    q["W6"], q["b6"] = np.zeros_like(q["W6"]), None
    h, _ = R.transformer_layer(s, t, n, x, e, q)
    ref = AL.transformer_conv(s + 1, t + 1, n, x, q["W1"], q["b1"], q["W2"], q["b2"], q["W3"], q["b3"], q["W4"], q["b4"], heads=2,
                              concat=concat)
    assert R.rel(ref, h) <= 1e-5


def test_the_gpu_graph_is_what_the_gpu_tests_say():
    R.assert_graph(*R.graph())
