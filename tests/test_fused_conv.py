"""The fused aggregate-then-transform kernel (csrc/fused_conv.hip, gnnmp_fused_conv_f32) against the unfused HIP path and
the oracle:
  * the pre-GEMM aggregate it forms in LDS (returned through the optional agg_out) is BIT-IDENTICAL to gnnmp_propagate_f32 /
    gnnmp_propagate_slots_f32 on the same plan — every aggr, scaled and not, rows the plan splits included;
  * the layer output is within 1e-5 of the oracle's layer body (GNNlib/src/layers/conv.jl:59-71,102-108,277-283) and of the
    unfused propagate + dense composition;
  * repeated launches (the self re-arming tile ticket), shapes outside the envelope (fallback), bipartite inputs."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
RTOL = 1e-5


@pytest.fixture(scope="module")
def gm():
    import torch
    assert torch.cuda.is_available()
    import gnnmp
    gnnmp.load()
    # the library only fuses when the aggregate cannot stay in the Infinity Cache (>= 128 MB); these graphs are small, so
    # force the fused kernel for the whole module (knob 14 > 0 = cap of waves per block, 16 = the automatic maximum)
    with gnnmp.tuned(gnnmp.Knob.FUSED_WAVES, 16):
        yield gnnmp


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def close(got, ref, rtol=RTOL):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape
    assert np.linalg.norm(got - ref) <= rtol * np.linalg.norm(ref) + 1e-30
    assert np.abs(got - ref).max() <= rtol * np.abs(ref).max() + 1e-30      # element-wise against the array scale, k = 1 (round 6; 4 before)


def hub_graph(rng, n=3000, E=40000, hub_edges=(700, 1500, 90)):
    """random multigraph + hubs above both split thresholds (64 on small graphs, 512) + isolated destinations"""
    s = [rng.integers(1, n - 40, E)]
    t = [rng.integers(1, n - 40, E)]
    for k, m in enumerate(hub_edges):
        s.append(rng.integers(1, n - 40, m))
        t.append(np.full(m, 7 + 13 * k))
    s, t = np.concatenate(s), np.concatenate(t)
    p = rng.permutation(len(s))
    return s[p].astype(np.int64), t[p].astype(np.int64), n


@pytest.mark.parametrize("D,Dout", [(100, 100), (128, 128), (12, 20), (64, 8), (4, 4), (16, 128), (100, 36), (52, 100)])
def test_aggregate_is_bit_identical_and_output_matches(gm, oracle, D, Dout):
    import torch
    from gnnmp import _lib as L
    rng = np.random.default_rng(D * 131 + Dout)
    s, t, n = hub_graph(rng)
    x = rng.standard_normal((n, D)).astype(np.float32)
    W = (rng.standard_normal((Dout, D)) * 0.2).astype(np.float32)
    b = (rng.standard_normal(Dout) * 0.1).astype(np.float32)
    w = (rng.random(len(s)) + 0.1).astype(np.float32)
    g = gm.GNNGraph(dev(s), dev(t), dev(w), num_nodes=n)
    xd, Wd, bd = dev(x), dev(W), dev(b)
    for loops in (False, True):
        plan = g.plan(loops)
        for aggr, name in ((L.SUM, "+"), (L.MEAN, "mean"), (L.MAX, "max"), (L.MIN, "min")):
            res = gm.fused_conv(plan, aggr, xd, Wd, bd, "relu", return_aggregate=True)
            assert res is not None, "this shape is inside the fused kernel's envelope"
            y, agg = res
            ref_agg = torch.empty_like(agg)
            L.check(L.load().gnnmp_propagate_f32(plan.handle, L.COPY_XJ, aggr, L.ptr(xd), None, None, None, L.ptr(ref_agg), D,
                                                 L.stream_ptr()))
            assert torch.equal(agg, ref_agg), f"aggregate differs from the unfused kernel (aggr {name}, loops {loops})"
            y_ref = gm.dense(ref_agg, Wd, bd, "relu")
            fin = torch.isfinite(y_ref).all(1) & torch.isfinite(ref_agg).all(1)      # max/min of empty rows: -Inf/+Inf, both paths
            close(y[fin].cpu().numpy(), y_ref[fin].cpu().numpy())
            assert torch.equal(torch.isfinite(y).all(1), torch.isfinite(y_ref).all(1))
            # twice: same bits (no atomics on the data path; the ticket only changes who computes a tile)
            assert torch.allclose(gm.fused_conv(plan, aggr, xd, Wd, bd, "relu"), y, rtol=0, atol=0, equal_nan=True)
        # scaled sum (GCN's normalisation): per-edge weights + source / destination factors
        c = dev((rng.random(n) + 0.5).astype(np.float32))
        wfull = g.w
        y, agg = gm.fused_conv(plan, L.SUM, xd, Wd, bd, None, w=wfull, scale_src=c, scale_dst=c, return_aggregate=True)
        ref_agg = torch.empty_like(agg)
        L.check(L.load().gnnmp_propagate_f32(plan.handle, L.W_MUL_XJ, L.SUM, L.ptr(xd), L.ptr(wfull), L.ptr(c), L.ptr(c),
                                             L.ptr(ref_agg), D, L.stream_ptr()))
        assert torch.equal(agg, ref_agg)
        close(y.cpu().numpy(), gm.dense(ref_agg, Wd, bd).cpu().numpy())
    # against the oracle, unscaled sum without loops
    ref = oracle.matmul(W, oracle.propagate("+", s, t, n, x)) + b[None, :]
    close(gm.fused_conv(g.plan(False), L.SUM, xd, Wd, bd).cpu().numpy(), ref)


@pytest.mark.parametrize("D1,D,Dout", [(100, 100, 128), (16, 16, 128), (12, 12, 20), (8, 24, 64)])
def test_root_segment(gm, oracle, D1, D, Dout):
    """W_root * x_i + W_agg * aggregate (graph_conv / sage_conv, conv.jl:102-108,277-283), bipartite source / destination sets"""
    import torch
    from gnnmp import _lib as L
    rng = np.random.default_rng(D1 + 7 * D + Dout)
    n_src, n_dst, E = 500, 333, 6000
    s, t = rng.integers(1, n_src + 1, E).astype(np.int64), rng.integers(1, n_dst + 1, E).astype(np.int64)
    from gnnmp.graph import Plan
    plan = Plan(dev(s), dev(t), n_src, n_dst, 1, False)
    xj = rng.standard_normal((n_src, D)).astype(np.float32)
    xi = rng.standard_normal((n_dst, D1)).astype(np.float32)
    W1 = (rng.standard_normal((Dout, D1)) * 0.2).astype(np.float32)
    W2 = (rng.standard_normal((Dout, D)) * 0.2).astype(np.float32)
    b = (rng.standard_normal(Dout) * 0.1).astype(np.float32)
    for aggr, name in ((L.SUM, "+"), (L.MEAN, "mean")):
        y = gm.fused_conv(plan, aggr, dev(xj), dev(W2), dev(b), "relu", xi=dev(xi), W_root=dev(W1))
        assert y is not None
        m = oracle.propagate(name, s, t, n_src, xj, n_dst=n_dst)
        ref = oracle._act("relu", oracle.matmul(W1, xi) + oracle.matmul(W2, m) + b[None, :])
        close(y.cpu().numpy(), ref)


@pytest.mark.parametrize("variant", [16, 8])
@pytest.mark.parametrize("Dout", [256, 384])
def test_sage_fused_cat_kernel(gm, oracle, variant, Dout):
    """fused_cat_kernel (round 6, BASELINE config 4): sage_conv / graph_conv 100 + 100 => 256 in ONE kernel, W streamed from L2 as
    pre-split bf16 planes (conv.jl:277-283,102-108).  The pre-GEMM aggregate is BIT-IDENTICAL to gnnmp_propagate_f32 for every aggr
    (split hubs included), the output within 1e-5 of the oracle and of the two-kernel path, non-finite rows (empty max / min rows, NaN
    and Inf features) come out exactly like the two-kernel path's.  variant = knob 14: 12 waves a block, or 8."""
    import torch
    from gnnmp import _lib as L
    from gnnmp.graph import Plan
    rng = np.random.default_rng(Dout + variant)
    s, t, n = hub_graph(rng, n=2500, E=30000)
    D = 100
    xj = rng.standard_normal((n, D)).astype(np.float32)
    W1 = (rng.standard_normal((Dout, D)) * 0.2).astype(np.float32)
    W2 = (rng.standard_normal((Dout, D)) * 0.2).astype(np.float32)
    b = (rng.standard_normal(Dout) * 0.1).astype(np.float32)
    g = gm.GNNGraph(dev(s), dev(t), num_nodes=n)
    plan = g.plan(False)
    assert plan.n_long >= 2
    xd, W1d, W2d, bd = dev(xj), dev(W1), dev(W2), dev(b)
    with gm.tuned(gm.Knob.FUSED_WAVES, variant):
        for aggr, name in ((L.SUM, "+"), (L.MEAN, "mean"), (L.MAX, "max"), (L.MIN, "min")):
            res = gm.fused_conv(plan, aggr, xd, W2d, bd, "relu", xi=xd, W_root=W1d, return_aggregate=True)
            assert res is not None, "100 + 100 => a multiple of 128 is inside fused_cat_kernel's envelope"
            y, agg = res
            ref_agg = torch.empty_like(agg)
            L.check(L.load().gnnmp_propagate_f32(plan.handle, L.COPY_XJ, aggr, L.ptr(xd), None, None, None, L.ptr(ref_agg), D, L.stream_ptr()))
            assert torch.equal(agg, ref_agg), f"aggregate differs from the unfused kernel (aggr {name})"
            y_ref = gm.dense(xd, W1d, bd, "relu", x2=ref_agg, W2=W2d)
            fin = torch.isfinite(ref_agg).all(1)
            close(y[fin].cpu().numpy(), y_ref[fin].cpu().numpy())
            # rows whose aggregate is -Inf / +Inf (no incoming edge under max / min): the exact path, same non-finite pattern
            assert torch.equal(torch.isnan(y), torch.isnan(y_ref)) and torch.equal(torch.isinf(y), torch.isinf(y_ref))
            assert torch.equal(gm.fused_conv(plan, aggr, xd, W2d, bd, "relu", xi=xd, W_root=W1d).view(torch.int32), y.view(torch.int32))
            if name in ("+", "mean"):
                m = oracle.propagate(name, s, t, n, xj)
                ref = oracle._act("relu", oracle.matmul(W1, xj) + oracle.matmul(W2, m) + b[None, :])
                close(y.cpu().numpy(), ref)
        # Inf / NaN features: the tiles that see them are redone in exact fp32; every other row is untouched
        xbad = xj.copy()
        xbad[17, 3] = np.inf
        xbad[900, 50] = np.nan
        xbad[1500, 99] = -np.inf
        xb = dev(xbad)
        y = gm.fused_conv(plan, L.SUM, xb, W2d, bd, None, xi=xb, W_root=W1d)
        aggb = torch.empty_like(xb)
        L.check(L.load().gnnmp_propagate_f32(plan.handle, L.COPY_XJ, L.SUM, L.ptr(xb), None, None, None, L.ptr(aggb), D, L.stream_ptr()))
        y_ref = gm.dense(xb, W1d, bd, None, x2=aggb, W2=W2d)
        assert torch.equal(torch.isnan(y), torch.isnan(y_ref)) and torch.equal(torch.isinf(y), torch.isinf(y_ref))
        fin = torch.isfinite(y_ref)
        assert fin.any() and not fin.all()
        d = (y[fin] - y_ref[fin]).abs().max().item()
        assert d <= 1e-5 * y_ref[fin].abs().max().item()
        # the layer itself takes the kernel (sage_conv: W * vcat(x_i, m))
        l = gm.SAGEConv((D, Dout), "relu", aggr="mean", seed=5)
        yl = l(g, xd).cpu().numpy()
        ref = oracle.sage_conv(s, t, n, xj, l.weight.cpu().numpy(), l.bias.cpu().numpy(), "relu", "mean")
        close(yl, ref)


def test_layers_take_the_fused_kernel_and_fall_back_outside_it(gm, oracle):
    import torch
    rng = np.random.default_rng(77)
    s, t, n = hub_graph(rng, n=1200, E=15000)
    g = gm.GNNGraph(dev(s), dev(t), num_nodes=n)
    from gnnmp import _lib as L
    # outside the envelope: D = 3 (not a multiple of 4), Dout = 132 > 128, Dout = 5
    for D, Dout in ((3, 8), (8, 132), (8, 5)):
        x = dev(rng.standard_normal((n, D)).astype(np.float32))
        W = dev(rng.standard_normal((Dout, D)).astype(np.float32))
        assert gm.fused_conv(g.plan(False), L.SUM, x, W) is None
    # the layers give the oracle's answer on either side of the boundary
    for Din, Dout in ((8, 16), (3, 16), (8, 132)):
        x = rng.standard_normal((n, Din)).astype(np.float32)
        for cls, orc in ((gm.GCNConv, "gcn"), (gm.SAGEConv, "sage"), (gm.GraphConv, "graph")):
            l = cls((Din, Dout), "relu", seed=5)
            y = l(g, dev(x)).cpu().numpy()
            if orc == "gcn":
                ref = oracle.gcn_conv(s, t, n, x, l.weight.cpu().numpy(), l.bias.cpu().numpy(), "relu")
            elif orc == "sage":
                ref = oracle.sage_conv(s, t, n, x, l.weight.cpu().numpy(), l.bias.cpu().numpy(), "relu", "mean")
            else:
                ref = oracle.graph_conv(s, t, n, x, l.weight1.cpu().numpy(), l.weight2.cpu().numpy(), l.bias.cpu().numpy(), "relu", "+")
            close(y, ref)


def test_many_launches_start_from_a_zeroed_ticket(gm):
    """200 back-to-back launches on one plan, alternating shapes: every one must see a zeroed ticket"""
    import torch
    from gnnmp import _lib as L
    rng = np.random.default_rng(3)
    s, t, n = hub_graph(rng, n=5000, E=60000)
    g = gm.GNNGraph(dev(s), dev(t), num_nodes=n)
    plan = g.plan(True)
    xa, xb = dev(rng.standard_normal((n, 100)).astype(np.float32)), dev(rng.standard_normal((n, 16)).astype(np.float32))
    Wa, Wb = dev(rng.standard_normal((100, 100)).astype(np.float32) * 0.1), dev(rng.standard_normal((32, 16)).astype(np.float32))
    ya, yb = gm.fused_conv(plan, L.SUM, xa, Wa), gm.fused_conv(plan, L.MEAN, xb, Wb)
    for _ in range(100):
        assert torch.equal(gm.fused_conv(plan, L.SUM, xa, Wa), ya)
        assert torch.equal(gm.fused_conv(plan, L.MEAN, xb, Wb), yb)


@pytest.mark.parametrize("Din,Dout", [(100, 100), (16, 128), (128, 128), (12, 20)])
def test_gcn_layer_adjoint_through_the_fused_kernels(gm, oracle, Din, Dout):
    """gcn_conv_ad with the fused kernel forced (module fixture): the forward hands out the aggregate next to the output, the
    backward forms Δx = PT(Δz) * W as ONE aggregate-then-transform on the plan of the reversed edges (w_layout = 1).  Against
    the oracle's composition of NNlib's rules (FD-pinned on CPU), hubs above the split threshold included."""
    import torch
    from gnnmp.backward import gcn_conv_ad
    rng = np.random.default_rng(Din * 7 + Dout)
    s, t, n = hub_graph(rng, n=1500, E=20000, hub_edges=(600, 90))
    x = rng.standard_normal((n, Din)).astype(np.float32)
    r = rng.standard_normal((n, Dout)).astype(np.float32)
    g = gm.GNNGraph(dev(s), dev(t), num_nodes=n)
    l = gm.GCNConv((Din, Dout), "relu", seed=5)
    l.bias = dev(rng.standard_normal(Dout).astype(np.float32) * 0.1)
    W0, b0 = l.weight.cpu().numpy(), l.bias.cpu().numpy()
    xt = dev(x).requires_grad_(True)
    l.weight.requires_grad_(True)
    l.bias.requires_grad_(True)
    y = gcn_conv_ad(l, g, xt)
    ref_y = oracle.gcn_conv(s, t, n, x, W0, b0, "relu")
    assert np.linalg.norm(y.detach().cpu().numpy() - ref_y) <= 1e-5 * np.linalg.norm(ref_y)
    (y * dev(r)).sum().backward()
    dx, dW, db = oracle.grad_gcn_conv(s, t, n, x, W0, b0, "relu", r)
    for got, ref in ((xt.grad, dx), (l.weight.grad, dW), (l.bias.grad, db)):
        assert np.linalg.norm(got.cpu().numpy() - ref) <= 1e-5 * np.linalg.norm(ref)
    # and the same gradients as the unfused composition
    with gm.tuned(gm.Knob.FUSED_WAVES, -1):
        x2 = dev(x).requires_grad_(True)
        l.weight.grad = None
        l.bias.grad = None
        y2 = gcn_conv_ad(l, g, x2)
        (y2 * dev(r)).sum().backward()
    close(xt.grad.cpu().numpy(), x2.grad.cpu().numpy(), 1e-5)
    close(y.detach().cpu().numpy(), y2.detach().cpu().numpy())


@pytest.mark.parametrize("log2g", [3, 6])
def test_a_forced_lane_group_is_refused_and_the_layer_falls_back(gm, oracle, log2g):
    """fused_conv_kernel has no feature tiles: with FORCE_LOG2G below ceil(log2(D / 4)) the features beyond 4 G would never reach the
    LDS tile the MFMA phase contracts over.  The export refuses any forced width other than its own (csrc/knobs.h, knob 1) before it
    writes anything, and the layer takes propagate + dense."""
    import torch
    from gnnmp import _lib as L
    rng = np.random.default_rng(41)
    s, t, n = hub_graph(rng, n=1200, E=15000)
    D = Dout = 100
    x = rng.standard_normal((n, D)).astype(np.float32)
    g = gm.GNNGraph(dev(s), dev(t), num_nodes=n)
    l = gm.GCNConv((D, Dout), "relu", seed=5)
    ref = oracle.gcn_conv(s, t, n, x, l.weight.cpu().numpy(), l.bias.cpu().numpy(), "relu")
    close(l(g, dev(x)).cpu().numpy(), ref)                        # the fused kernel (module fixture: FUSED_WAVES = 16)
    with gm.tuned(gm.Knob.FORCE_LOG2G, log2g):
        close(l(g, dev(x)).cpu().numpy(), ref)                    # the same layer with the group forced
        # the raw export: GNNMP_EUNSUPPORTED, and neither output touched
        xd, W = dev(x), dev((rng.standard_normal((Dout, D)) * 0.2).astype(np.float32))
        poison = float(np.frombuffer(np.uint32(0x7fc0beef).tobytes(), np.float32)[0])
        out, agg = torch.full((n, Dout), poison, device="cuda"), torch.full((n, D), poison, device="cuda")
        before_out, before_agg = out.view(torch.int32).clone(), agg.view(torch.int32).clone()
        rc = L.load().gnnmp_fused_conv_f32(g.plan(False).handle, L.SUM, L.ptr(xd), None, None, None, None, None, D, None, 0, None, 0,
                                           L.ptr(W), W.stride(0), 0, None, 0, L.ptr(out), Dout, L.ptr(agg), L.stream_ptr())
        torch.cuda.synchronize()
        assert rc == L.EUNSUPPORTED
        assert torch.equal(out.view(torch.int32), before_out) and torch.equal(agg.view(torch.int32), before_agg)
        assert gm.fused_conv(g.plan(False), L.SUM, xd, W) is None
    assert gm.fused_conv(g.plan(False), L.SUM, xd, W) is not None      # the knob is back: the kernel takes the shape again
