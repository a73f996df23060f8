"""gated_graph_conv_ad and res_gated_graph_conv_ad: the two gated layers trained on libgnnmp (gnnmp/backward_gated.py), and one training
step of a small model built from the new functions.  The exports they stand on are tested in tests/test_poly_conv_ad.py
(gnnmp_gru_pointwise_grad_f32) and tests/test_cg_conv_ad.py (gnnmp_cg_conv_grad_f32).

Without a GPU: the float64 models (tests/gated_conv_ref.py) agree with central finite differences in every argument, for all four folds,
and with oracle.more_layers.gated_graph_conv / oracle.khop_layers.res_gated_graph_conv; the operands of every GPU case keep the float32
restatement within 2e-6 of float64, relu's pre-activations 1e-3 from 0 and max / min's winners 1e-3 ahead — but for one deliberate exact
tie (a repeated edge).

On the GPU: the forwards bit for bit the existing forwards and within 1e-5 of float64; every gradient (dx at 1e-5; weights and biases
inside γ_n Σ|terms|, n as tests/gated_conv_ref.py: sum_n reasons); pruning; refusals; ChebConv -> GatedGraphConv -> global_pool_ad -> loss
against the float64 model, gradients and the loss after one SGD step."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gated_conv_ref as R  # noqa: E402
import poly_conv_ref as P  # noqa: E402

gpu = pytest.mark.gpu
f32, f64 = np.float32, np.float64


def _c(a, dtype=f64):
    return None if a is None else a.astype(dtype)


# ------------------------------------------------------------------------------------------------------------------------------------
# CPU: the references
# ------------------------------------------------------------------------------------------------------------------------------------
def fd_check(loss, operands, h=1e-6):
    """central differences of `loss()` in every element of every (array, gradient, name)"""
    for arr, g, what in operands:
        fd = np.zeros_like(arr)
        for i in np.ndindex(arr.shape):
            keep = arr[i]
            arr[i] = keep + h
            hi = loss()
            arr[i] = keep - h
            lo = loss()
            arr[i] = keep
            fd[i] = (hi - lo) / (2 * h)
        assert np.abs(fd - g).max() <= 1e-6 * max(np.abs(g).max(), 1.0), (what, np.abs(fd - g).max())


@pytest.mark.parametrize("layers", [1, 3])
@pytest.mark.parametrize("aggr", R.AGGRS)
def test_gated_graph_conv_reference_gradient_agrees_with_finite_differences(aggr, layers):
    """x, weight, Wi, Wh and b of the float64 model, h = 1e-6.  The repeated edge is left out here: where two copies of one message tie,
    the reference's rule (every copy gets Δ) is not the derivative of max; the winners' leads (>= 1e-3, the condition below) keep every
    other comparison more than 100 h from its kink"""
    s, t, (k1, k2) = R.layer_graph()
    s, t = np.delete(s, k2), np.delete(t, k2)
    x, W, Wi, Wh, b, dY = [_c(a) for a in R.ggc_case(aggr, 4, layers)]
    ref = R.ggc_grad(s, t, R.N_NODES, x, W, Wi, Wh, b, aggr, dY)
    fd_check(lambda: float((R.ggc_forward(s, t, R.N_NODES, x, W, Wi, Wh, b, aggr) * dY).sum()),
             [(x, ref["dx"], "dx"), (W, ref["dW"], "dW"), (Wi, ref["dWi"], "dWi"), (Wh, ref["dWh"], "dWh"), (b, ref["db"], "db")])


@pytest.mark.parametrize("sigma,bias", R.RGC_CASES)
def test_res_gated_reference_gradient_agrees_with_finite_differences(sigma, bias):
    s, t, _ = R.layer_graph()
    x, A, B, U, V, bv, dY = [_c(a) for a in R.rgc_case(sigma, bias)]
    ref = R.rgc_grad(s, t, R.N_NODES, x, A, B, U, V, bv, sigma, dY)
    ops = [(x, ref["dx"], "dx"), (A, ref["dA"], "dA"), (B, ref["dB"], "dB"), (U, ref["dU"], "dU"), (V, ref["dV"], "dV")]
    fd_check(lambda: float((R.rgc_forward(s, t, R.N_NODES, x, A, B, U, V, bv, sigma) * dY).sum()), ops + ([(bv, ref["db"], "db")] if bias else []))


def _close64(got, ref, tol=1e-5):
    got, ref = np.asarray(got, f64), np.asarray(ref, f64)
    return np.linalg.norm(got - ref) <= tol * np.linalg.norm(ref) and np.abs(got - ref).max() <= tol * np.abs(ref).max()


@pytest.mark.parametrize("aggr,m,layers", R.GGC_CASES)
def test_gated_graph_conv_reference_agrees_with_the_oracle(aggr, m, layers):
    from oracle import more_layers as ML
    s, t, _ = R.layer_graph()
    x, W, Wi, Wh, b, _ = R.ggc_case(aggr, m, layers)
    assert _close64(ML.gated_graph_conv(s + 1, t + 1, R.N_NODES, x, W, Wi, Wh, b, aggr=aggr), R.ggc_ref(aggr, m, layers)["Y"])


@pytest.mark.parametrize("sigma,bias", R.RGC_CASES)
def test_res_gated_reference_agrees_with_the_oracle(sigma, bias):
    from oracle import khop_layers as KL
    s, t, _ = R.layer_graph()
    x, A, B, U, V, bv, _ = R.rgc_case(sigma, bias)
    assert _close64(KL.res_gated_graph_conv(s + 1, t + 1, R.N_NODES, x, A, B, U, V, bv, sigma), R.rgc_ref(sigma, bias)["Y"])


@pytest.mark.parametrize("aggr,m,layers", R.GGC_CASES)
def test_the_gated_graph_conv_cases_are_well_conditioned(aggr, m, layers):
    """THE CONDITION ON THE INPUTS, not a measurement"""
    worst, lead = R.ggc_condition(aggr, m, layers)
    assert worst <= R.COND, f"the float32 restatement is {worst:.2e} from float64 (bound {R.COND:g})"
    assert lead >= R.KINK, f"a winner leads by only {lead:.2e}"
    s, t, (k1, k2) = R.layer_graph()
    assert s[k1] == s[k2] and t[k1] == t[k2] and k1 != k2      # the deliberate tie: two copies of one message
    assert np.bincount(t, minlength=R.N_NODES).min() >= 1      # no empty row: max / min stay finite


@pytest.mark.parametrize("sigma,bias", R.RGC_CASES)
def test_the_res_gated_cases_are_well_conditioned(sigma, bias):
    worst, kink = R.rgc_condition(sigma, bias)
    assert worst <= R.COND and kink >= R.KINK, (worst, kink)


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------------------------------------------
def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def close(got, ref, what, tol=1e-5):
    """the project's parity bar, norm-wise AND element-wise against the array scale"""
    got, ref = np.asarray(got, f64), np.asarray(ref, f64)
    assert got.shape == ref.shape, what
    assert np.all(np.isfinite(got)), f"{what}: non-finite"
    err, scale = np.linalg.norm(got - ref), np.linalg.norm(ref)
    worst = np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300) if ref.size else 0.0
    print(f"{what}: |got - ref| = {err:.3e}, |ref| = {scale:.3e}, ratio {err / max(scale, 1e-300):.2e}, element-wise {worst:.2e}")
    assert err <= tol * scale, f"{what}: {err:.3e} > {tol:g} * {scale:.3e}"
    assert worst <= tol, f"{what}: element-wise {worst:.2e} of the array scale"


def within_sum_bound(got, ref, mag, n, what):
    """|got − ref64| <= γ_n Σ|terms|, element-wise"""
    got, ref = np.asarray(got, f64), np.asarray(ref, f64)
    assert got.shape == ref.shape and np.all(np.isfinite(got)), what
    bound = R.gamma(n) * mag
    used = float((np.abs(got - ref) / np.maximum(bound, 1e-300)).max()) if got.size else 0.0
    print(f"{what}: uses {used:.3f} of the summation bound (n = {n})")
    assert np.all(np.abs(got - ref) <= bound), f"{what}: {used:.2f} of the summation bound"


@pytest.fixture(scope="module")
def graph():
    import torch
    assert torch.cuda.is_available()
    import gnnmp
    s, t, _ = R.layer_graph()
    return gnnmp.GNNGraph(dev(s), dev(t), num_nodes=R.N_NODES, index_base=0)


def ggc_layer(aggr, m, layers):
    import gnnmp
    x, W, Wi, Wh, b, dY = R.ggc_case(aggr, m, layers)
    l = gnnmp.GatedGraphConv(R.GGC_DIMS, layers, aggr=aggr)
    l.weight, l.gru_Wi, l.gru_Wh, l.gru_b = dev(W), dev(Wi), dev(Wh), dev(b)
    return l, x, dY


def ggc_params(l):
    return [l.weight, l.gru_Wi, l.gru_Wh, l.gru_b]


@gpu
@pytest.mark.parametrize("aggr,m,layers", R.GGC_CASES)
def test_gated_graph_conv_ad(graph, aggr, m, layers):
    """forward: gnnmp.gated_graph_conv bit for bit (with and without a graph being recorded) and within 1e-5 of float64; dx within 1e-5
    (under max / min BOTH copies of the tied message send Δ back); weight, Wi, Wh, b inside γ_n Σ|terms|"""
    import torch
    import gnnmp
    l, x, dY = ggc_layer(aggr, m, layers)
    ref = R.ggc_ref(aggr, m, layers)
    with torch.no_grad():
        plain = gnnmp.gated_graph_conv(l, graph, dev(x))
        y0 = gnnmp.gated_graph_conv_ad(l, graph, dev(x))
    assert torch.equal(y0, plain)
    close(y0.cpu().numpy(), ref["Y"], "Y")
    xt = dev(x).requires_grad_(True)
    for p in ggc_params(l):
        p.requires_grad_(True)
        p.grad = None
    y = gnnmp.gated_graph_conv_ad(l, graph, xt)
    assert torch.equal(y.detach(), plain)
    y.backward(dev(dY))
    torch.cuda.synchronize()
    close(xt.grad.cpu().numpy(), ref["dx"], "dx")
    n = R.sum_n(R.N_NODES, R.N_EDGES, R.GGC_DIMS, layers)
    for p, key in zip(ggc_params(l), ("W", "Wi", "Wh", "b")):
        within_sum_bound(p.grad.cpu().numpy(), ref["d" + key], ref["mag_" + key], n, "d" + key)


def rgc_layer(sigma, bias):
    import gnnmp
    x, A, B, U, V, bv, dY = R.rgc_case(sigma, bias)
    l = gnnmp.ResGatedGraphConv(R.RGC_SHAPE, sigma, bias=bias)
    l.A, l.B, l.U, l.V = dev(A), dev(B), dev(U), dev(V)
    if bias:
        l.bias = dev(bv)
    return l, x, dY


def rgc_params(l):
    return [l.A, l.B, l.U, l.V] + ([l.bias] if l.bias is not None else [])


@gpu
@pytest.mark.parametrize("sigma,bias", R.RGC_CASES)
def test_res_gated_graph_conv_ad(graph, sigma, bias):
    """forward: gnnmp.res_gated_graph_conv bit for bit and within 1e-5 of float64; dx within 1e-5; A, B, U, V, bias inside γ_n Σ|terms|"""
    import torch
    import gnnmp
    l, x, dY = rgc_layer(sigma, bias)
    ref = R.rgc_ref(sigma, bias)
    with torch.no_grad():
        plain = gnnmp.res_gated_graph_conv(l, graph, dev(x))
        y0 = gnnmp.res_gated_graph_conv_ad(l, graph, dev(x))
    assert torch.equal(y0, plain)
    close(y0.cpu().numpy(), ref["Y"], "Y")
    xt = dev(x).requires_grad_(True)
    for p in rgc_params(l):
        p.requires_grad_(True)
        p.grad = None
    y = gnnmp.res_gated_graph_conv_ad(l, graph, xt)
    assert torch.equal(y.detach(), plain)
    y.backward(dev(dY))
    torch.cuda.synchronize()
    close(xt.grad.cpu().numpy(), ref["dx"], "dx")
    n = R.sum_n(R.N_NODES, R.N_EDGES, R.RGC_SHAPE[0], 1)
    for p, key in zip(rgc_params(l), ("A", "B", "U", "V", "b")):
        within_sum_bound(p.grad.cpu().numpy(), ref["d" + key], ref["mag_" + key], n, "d" + key)


@gpu
def test_needs_input_grad_prunes(graph):
    """GatedGraphConv, only x: no weight gradient comes back and dx keeps its value; only gru_b: nothing is sent below the first layer (one
    fold pullback a layer but the first).  ResGatedGraphConv, only U and bias: the gated-message adjoint does not run"""
    import torch
    import gnnmp
    from gnnmp import backward_gated as B
    l, x, dY = ggc_layer("mean", 4, 3)
    ref = R.ggc_ref("mean", 4, 3)
    for p in ggc_params(l):
        p.requires_grad_(False)
        p.grad = None
    xt = dev(x).requires_grad_(True)
    gnnmp.gated_graph_conv_ad(l, graph, xt).backward(dev(dY))
    torch.cuda.synchronize()
    assert all(p.grad is None for p in ggc_params(l))
    close(xt.grad.cpu().numpy(), ref["dx"], "dx")
    folds, fold_fn = [], B.propagate_grad_xj
    B.propagate_grad_xj = lambda *a, **kw: folds.append(1) or fold_fn(*a, **kw)
    try:
        l.gru_b.requires_grad_(True)
        xt = dev(x)
        gnnmp.gated_graph_conv_ad(l, graph, xt).backward(dev(dY))
        torch.cuda.synchronize()
    finally:
        B.propagate_grad_xj = fold_fn
    assert len(folds) == 2 and xt.grad is None and l.weight.grad is None and l.gru_Wi.grad is None
    within_sum_bound(l.gru_b.grad.cpu().numpy(), ref["db"], ref["mag_b"], R.sum_n(R.N_NODES, R.N_EDGES, R.GGC_DIMS, 3), "db")
    lr, xr, dYr = rgc_layer("relu", True)
    rows, rows_fn = [], B.cg_rows_grad
    B.cg_rows_grad = lambda *a, **kw: rows.append(1) or rows_fn(*a, **kw)
    try:
        for p in (lr.U, lr.bias):
            p.requires_grad_(True)
        gnnmp.res_gated_graph_conv_ad(lr, graph, dev(xr)).backward(dev(dYr))
        torch.cuda.synchronize()
    finally:
        B.cg_rows_grad = rows_fn
    assert not rows and lr.A.grad is None and lr.B.grad is None and lr.V.grad is None
    refr = R.rgc_ref("relu", True)
    n = R.sum_n(R.N_NODES, R.N_EDGES, R.RGC_SHAPE[0], 1)
    within_sum_bound(lr.U.grad.cpu().numpy(), refr["dU"], refr["mag_U"], n, "dU")
    within_sum_bound(lr.bias.grad.cpu().numpy(), refr["db"], refr["mag_b"], n, "db")


@gpu
def test_the_gated_layers_refuse_by_name(graph):
    import torch
    import gnnmp
    l, x, _ = ggc_layer("+", 4, 1)
    xt = dev(x)
    with pytest.raises(NotImplementedError, match="gated_graph_conv_ad: a bipartite"):
        gnnmp.gated_graph_conv_ad(l, graph, (xt, xt))
    with pytest.raises(ValueError, match="gated_graph_conv_ad: the HIP adjoints are Float32"):
        gnnmp.gated_graph_conv_ad(l, graph, xt.double())
    with pytest.raises(ValueError, match="gated_graph_conv_ad: number of input features"):
        gnnmp.gated_graph_conv_ad(l, graph, dev(np.zeros((R.N_NODES, R.GGC_DIMS + 1), f32)))
    lr, xr, _ = rgc_layer(None, True)
    xr = dev(xr)
    with pytest.raises(NotImplementedError, match="res_gated_graph_conv_ad: a bipartite"):
        gnnmp.res_gated_graph_conv_ad(lr, graph, (xr, xr))
    with pytest.raises(ValueError, match="res_gated_graph_conv_ad: the HIP adjoints are Float32"):
        gnnmp.res_gated_graph_conv_ad(lr, graph, xr.double())
    for sigma in ("tanh", "softplus", torch.sigmoid):
        lr.sigma = sigma
        with pytest.raises(ValueError, match="res_gated_graph_conv_ad: σ ="):
            gnnmp.res_gated_graph_conv_ad(lr, graph, xr)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU: a training step of a model built from the new functions
# ------------------------------------------------------------------------------------------------------------------------------------
def _model64(s, t, n, lam, x, Wc, bc, W, Wi, Wh, b, Rp):
    """(loss, Σ|terms| of the loss, gradients) of loss = Σ mean_nodes(GatedGraphConv(ChebConv(x))) ⊙ Rp, float64"""
    c = P.cheb_grad(s, t, n, x, Wc, bc, lam, np.zeros((n, Wc.shape[1])))      # the forward, and Z for the second pass
    gg = R.ggc_grad(s, t, n, c["Y"], W, Wi, Wh, b, "+", np.tile(Rp / n, (n, 1)))
    cg = P.cheb_grad(s, t, n, x, Wc, bc, lam, gg["dx"])
    loss, scale = float((gg["Y"].mean(0) * Rp).sum()), float(np.abs(gg["Y"].mean(0) * Rp).sum())
    return loss, scale, dict(Wc=cg["dW"], bc=cg["db"], W=gg["dW"], Wi=gg["dWi"], Wh=gg["dWh"], b=gg["db"])


@gpu
def test_one_training_step_of_a_cheb_gated_model():
    """ChebConv(12 => 6, k = 3) -> GatedGraphConv(6, 2 layers, +) -> global_pool_ad(mean) -> loss = Σ pooled ⊙ R on the bidirected graph of
    tests/poly_conv_ref.py: the loss and every parameter gradient within 1e-5 of the float64 model (the loss against the scale of its six terms, the gradients
    norm-wise), and the loss after one plain SGD step within 1e-5 of the float64 model's loss after ITS step"""
    import torch
    import gnnmp
    from gnnmp.backward import global_pool_ad
    s, t, n = P.bidirected_graph()
    rng = np.random.default_rng(51)
    x = rng.standard_normal((n, 12)).astype(f32)
    Wc = np.stack([P.glorot(rng, 6, 12) for _ in range(3)])
    bc = (0.1 * rng.standard_normal(6)).astype(f32)
    W = np.stack([P.glorot(rng, 6, 6) for _ in range(2)])
    Wi, Wh = P.glorot(rng, 18, 6), P.glorot(rng, 18, 6)
    b = (0.1 * rng.standard_normal(18)).astype(f32)
    Rp = rng.standard_normal(6).astype(f32)
    g = gnnmp.GNNGraph(dev(s), dev(t), num_nodes=n, index_base=0)
    cheb, ggc, pool = gnnmp.ChebConv((12, 6), 3), gnnmp.GatedGraphConv(6, 2), gnnmp.GlobalPool("mean")
    cheb.weight, cheb.bias = dev(Wc), dev(bc)
    ggc.weight, ggc.gru_Wi, ggc.gru_Wh, ggc.gru_b = dev(W), dev(Wi), dev(Wh), dev(b)
    params = dict(Wc=cheb.weight, bc=cheb.bias, W=ggc.weight, Wi=ggc.gru_Wi, Wh=ggc.gru_Wh, b=ggc.gru_b)
    for p in params.values():
        p.requires_grad_(True)
    lam = gnnmp.layers_more.scaled_laplacian_op(g)[3]
    xt, Rt = dev(x), dev(Rp)

    def loss():
        h = gnnmp.cheb_conv_ad(cheb, g, xt)
        h = gnnmp.gated_graph_conv_ad(ggc, g, h)
        return (global_pool_ad(pool, g, h) * Rt).sum()
    before = loss()
    before.backward()
    torch.cuda.synchronize()
    host = dict(Wc=Wc, bc=bc, W=W, Wi=Wi, Wh=Wh, b=b)
    c64 = {k: v.astype(f64) for k, v in host.items()}
    want, scale, grads = _model64(s, t, n, lam, x.astype(f64), c64["Wc"], c64["bc"], c64["W"], c64["Wi"], c64["Wh"], c64["b"], Rp.astype(f64))
    assert abs(float(before) - want) <= 1e-5 * scale, (float(before), want, scale)
    for k, p in params.items():
        got, ref = p.grad.cpu().numpy().astype(f64), grads[k]
        assert np.linalg.norm(got - ref) <= 1e-5 * np.linalg.norm(ref), (k, np.linalg.norm(got - ref) / np.linalg.norm(ref))
    lr = 0.05
    with torch.no_grad():
        for p in params.values():
            p -= lr * p.grad
        after = float(loss())
    stepped = {k: c64[k] - lr * grads[k] for k in c64}
    want_after, scale_after, _ = _model64(s, t, n, lam, x.astype(f64), stepped["Wc"], stepped["bc"], stepped["W"], stepped["Wi"], stepped["Wh"], stepped["b"],
                             Rp.astype(f64))
    print(f"loss {float(before):.6f} -> {after:.6f} (float64: {want:.6f} -> {want_after:.6f})")
    assert abs(after - want_after) <= 1e-5 * scale_after and want_after != want
