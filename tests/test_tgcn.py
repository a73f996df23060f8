"""TGCN (GraphNeuralNetworks/src/layers/temporalconv.jl:809-849 TGCNCell, :121-135 GNNRecurrence, :884 TGCN) against a float64
restatement of the reference, written statement by statement below, and torch float64 CPU autograd of it for every gradient.  The
restatement's GCN part is anchored against the oracle's gcn_conv in a CPU test.  Tolerance: the project's 1e-5, norm-wise AND
element-wise (tests/test_configs.py: close)."""
import ctypes
import math

import numpy as np
import pytest
import torch

RTOL = 1e-5


def close(got, ref, what="", rtol=RTOL):
    got = np.asarray(got.detach().cpu() if torch.is_tensor(got) else got, np.float64)
    ref = np.asarray(ref.detach().cpu() if torch.is_tensor(ref) else ref, np.float64)
    assert got.shape == ref.shape, what
    assert np.linalg.norm(got - ref) <= rtol * np.linalg.norm(ref) + 1e-30, f"{what}: norm-wise"
    worst = np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-30)
    assert worst <= rtol, f"{what}: element-wise {worst:.2e}"


# ---- the float64 restatement -------------------------------------------------------------------------------------------------------------
def ref_gcn(s, t, n, x, W, b, relu, loops, w=None):
    """GNNlib/src/layers/conv.jl:14-72 (s, t 0-based): self loops (weight 1), c = 1 ./ sqrt.(degree(g; dir = :in, edge_weight)), W first
    when out < in, x .* c', propagate(copy_xj | w_mul_xj, +), .* c', W after when out >= in, σ.(x .+ b)"""
    if loops:
        ar = torch.arange(n)
        s, t = torch.cat([s, ar]), torch.cat([t, ar])
        if w is not None:
            w = torch.cat([w, torch.ones(n, dtype=w.dtype)])
    ew = torch.ones(len(s), dtype=x.dtype) if w is None else w
    deg = torch.zeros(n, dtype=x.dtype).index_add(0, t, ew)
    c = 1.0 / torch.sqrt(deg)
    Dout, Din = W.shape
    if Dout < Din:
        x = x @ W.T
    x = x * c[:, None]
    xj = x[s] if w is None else x[s] * w[:, None]
    a = torch.zeros((n, x.shape[1]), dtype=x.dtype).index_add(0, t, xj)
    a = a * c[:, None]
    if Dout >= Din:
        a = a @ W.T
    if b is not None:
        a = a + b
    return torch.relu(a) if relu else a


def ref_tgcn(s, t, n, x, params, h0=None, loops=True, w=None):
    """GNNRecurrence(TGCNCell): scan over dims 2 of (in, T, N) = torch dim 1 of [N, T, in]; per step temporalconv.jl:840-849"""
    T = x.shape[1]
    out = params[4].shape[0]
    h = torch.zeros((n, out), dtype=x.dtype) if h0 is None else h0.expand(n, out)
    ys = []
    for step in range(T):
        xt = x[:, step]
        convs = []
        for k in range(3):
            W1, b1, W2, b2 = params[6 * k: 6 * k + 4]
            convs.append(ref_gcn(s, t, n, ref_gcn(s, t, n, xt, W1, b1, True, loops, w), W2, b2, False, loops, w))
        Wz, bz, Wr, br, Wh, bh = params[4], params[5], params[10], params[11], params[16], params[17]
        z = torch.sigmoid(torch.cat([convs[0], h], 1) @ Wz.T + bz)
        r = torch.sigmoid(torch.cat([convs[1], h], 1) @ Wr.T + br)
        ht = torch.tanh(torch.cat([convs[2], r * h], 1) @ Wh.T + bh)
        h = (1 - z) * h + z * ht
        ys.append(h)
    return torch.stack(ys, 1)


def rand_params(cin, cout, seed=0):
    """the 18 parameters of a TGCNCell in TGCNCell.parameters() order, float64"""
    g = torch.Generator().manual_seed(seed)
    ps = []
    for _ in range(3):
        for shape in ((cout, cin), (cout,), (cout, cout), (cout,), (cout, 2 * cout), (cout,)):
            sc = math.sqrt(6.0 / sum(shape)) if len(shape) == 2 else 0.3
            ps.append((torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 1) * sc)
    return ps


def small_graph(seed=0, n=6, m=10):
    from gnnmp import synth
    s, t = synth.rand_graph(n, m, np.random.default_rng(seed))
    return torch.from_numpy(s - 1), torch.from_numpy(t - 1), n


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------------
def test_new_entry_points_are_declared_and_exported():
    from gnnmp import _lib
    names = ("gnnmp_tgcn_recurrence_f32", "gnnmp_tgcn_recurrence_grad_f32", "gnnmp_tgcn_step_f32", "gnnmp_tgcn_step_grad_f32")
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gnnmp.h")).read()
    lib = _lib.load()
    for nm in names:
        assert nm in _lib.SYMBOLS and (nm + "(") in hdr
        assert hasattr(lib, nm)


def test_tgcn_argument_validation_needs_no_gpu():
    """bad sizes, NULL required pointers and out beyond the one-launch kernel's envelope: EINVAL before any HIP call"""
    from gnnmp import _lib
    lib = _lib.load()
    E = _lib.EINVAL
    p = ctypes.c_void_p(16)          # never dereferenced: every call below fails validation first
    assert lib.gnnmp_tgcn_recurrence_f32(p, p, p, None, 0, p, None, 4, 3, 129, None) == E
    assert b"out" in lib.gnnmp_last_error()
    assert lib.gnnmp_tgcn_recurrence_f32(p, p, p, None, 0, p, None, 4, 3, 0, None) == E
    assert lib.gnnmp_tgcn_recurrence_f32(p, p, p, None, 0, p, None, 4, 0, 5, None) == E
    assert lib.gnnmp_tgcn_recurrence_f32(p, p, p, None, 0, p, None, -1, 3, 5, None) == E
    assert lib.gnnmp_tgcn_recurrence_f32(None, p, p, None, 0, p, None, 4, 3, 5, None) == E
    assert lib.gnnmp_tgcn_recurrence_f32(p, None, p, None, 0, p, None, 4, 3, 5, None) == E
    assert lib.gnnmp_tgcn_recurrence_f32(p, p, p, None, 0, None, None, 4, 3, 5, None) == E
    assert lib.gnnmp_tgcn_recurrence_f32(p, p, p, p, 7, p, None, 4, 3, 5, None) == E          # h0_stride neither 0 nor out
    assert lib.gnnmp_tgcn_recurrence_grad_f32(p, p, p, p, p, None, 0, p, None, None, 4, 3, 200, None) == E
    assert lib.gnnmp_tgcn_recurrence_grad_f32(None, p, p, p, p, None, 0, p, None, None, 4, 3, 5, None) == E
    assert lib.gnnmp_tgcn_recurrence_grad_f32(p, p, None, p, p, None, 0, p, None, None, 4, 3, 5, None) == E
    assert lib.gnnmp_tgcn_recurrence_grad_f32(p, p, p, p, p, None, 0, None, None, None, 4, 3, 5, None) == E
    assert lib.gnnmp_tgcn_step_f32(2, p, p, p, 5, p, p, p, 4, 3, 0, 5, None) == E
    assert lib.gnnmp_tgcn_step_f32(0, p, p, p, 5, p, p, p, 4, 3, 3, 5, None) == E            # t outside [0, T)
    assert lib.gnnmp_tgcn_step_f32(1, p, p, p, 5, p, p, None, 4, 3, 0, 5, None) == E
    assert lib.gnnmp_tgcn_step_grad_f32(0, None, None, p, p, 5, None, p, p, p, p, None, 4, 3, 0, 5, None) == E
    assert lib.gnnmp_tgcn_step_grad_f32(1, None, None, p, p, 5, None, p, None, p, p, None, 4, 3, 0, 5, None) == E
    # N = 0 is a valid empty call
    assert lib.gnnmp_tgcn_recurrence_f32(None, None, None, None, 0, None, None, 0, 3, 5, None) == _lib.OK


def test_restatement_gcn_matches_the_oracle(oracle):
    rng = np.random.default_rng(3)
    for (cin, cout, loops, use_w) in ((3, 5, True, False), (16, 8, True, False), (4, 4, False, False), (5, 7, True, True)):
        s1, t1 = (np.array([1, 2, 3, 4, 5, 6, 2, 1, 6, 3]), np.array([2, 3, 4, 5, 6, 1, 1, 3, 2, 5]))
        n = 6
        x = rng.standard_normal((n, cin)).astype(np.float32)
        W = rng.standard_normal((cout, cin)).astype(np.float32)
        b = rng.standard_normal(cout).astype(np.float32)
        w = rng.random(len(s1)).astype(np.float32) + 0.5 if use_w else None
        ref = oracle.gcn_conv(s1, t1, n, x, W, b, "relu", add_self_loops_=loops, use_edge_weight=use_w, graph_w=w)
        got = ref_gcn(torch.from_numpy(s1 - 1), torch.from_numpy(t1 - 1), n, torch.from_numpy(x).double(), torch.from_numpy(W).double(),
                      torch.from_numpy(b).double(), True, loops, None if w is None else torch.from_numpy(w).double())
        close(got, ref, f"gcn {cin}=>{cout} loops={loops} w={use_w}")


def test_restatement_gradients_match_finite_differences():
    s, t, n = small_graph(1, 5, 8)
    ps = [p.requires_grad_() for p in rand_params(2, 3, seed=2)]
    x = torch.randn((n, 3, 2), dtype=torch.float64, requires_grad=True)
    h0 = torch.randn(3, dtype=torch.float64, requires_grad=True)
    assert torch.autograd.gradcheck(lambda x, h0, *ps: ref_tgcn(s, t, n, x, ps, h0), (x, h0, *ps), eps=1e-6, atol=1e-7, rtol=1e-5)


def test_layers_construct_on_cpu_with_the_reference_fields():
    import gnnmp
    cell = gnnmp.TGCNCell((3, 5), device="cpu", seed=1)
    assert (cell.in_, cell.out) == (3, 5)
    for g in "zrh":
        conv, d = getattr(cell, "conv_" + g), getattr(cell, "dense_" + g)
        assert isinstance(conv, gnnmp.GNNChain) and all(isinstance(l, gnnmp.GCNConv) for l in conv.layers)
        assert tuple(conv.layers[0].weight.shape) == (5, 3) and conv.layers[0].sigma == "relu"
        assert tuple(conv.layers[1].weight.shape) == (5, 5) and conv.layers[1].sigma is None
        assert isinstance(d, gnnmp.Dense) and tuple(d.weight.shape) == (5, 10) and tuple(d.bias.shape) == (5,)
    assert len(cell.parameters()) == 18
    assert tuple(cell.initialstates().shape) == (5,) and float(cell.initialstates().abs().sum()) == 0.0
    layer = gnnmp.TGCN((2, 100), device="cpu", bias=False, add_self_loops=False)
    assert isinstance(layer, gnnmp.GNNRecurrence) and layer.takes_graph and isinstance(layer.cell, gnnmp.TGCNCell)
    assert layer.cell.conv_h.layers[0].bias is None and not layer.cell.add_self_loops
    assert tuple(layer.cell.dense_h.weight.shape) == (100, 200)


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------
def road_graph(n, deg=8, seed=0):
    """a road-like graph: local chords to the next few nodes of a ring, bidirected, no self loops, duplicates removed; 1-based int64"""
    rng = np.random.default_rng(seed)
    src, dst = [], []
    for i in range(n):
        for _ in range(deg // 2):
            j = (i + int(rng.integers(1, 12))) % n
            if j != i:
                src += [i, j]
                dst += [j, i]
    e = np.unique(np.stack([src, dst], 1), axis=0)
    return e[:, 0].astype(np.int64) + 1, e[:, 1].astype(np.int64) + 1


def _run_case(s1, t1, n, cin, cout, T, state=None, bias=True, loops=True, w=None, grads=True, seed=0):
    import gnnmp
    dev = "cuda"
    g = gnnmp.GNNGraph(torch.from_numpy(s1).to(dev), torch.from_numpy(t1).to(dev),
                       w=None if w is None else torch.from_numpy(w).to(dev), num_nodes=n)
    layer = gnnmp.TGCN((cin, cout), bias=bias, add_self_loops=loops, use_edge_weight=w is not None, seed=seed)
    ps = [None if p is None else p.detach().cpu().double() for p in layer.cell.parameters()]
    rng = np.random.default_rng(seed + 1)
    x = torch.from_numpy(rng.standard_normal((n, T, cin)).astype(np.float32))
    s, t = torch.from_numpy(s1 - 1), torch.from_numpy(t1 - 1)
    wt = None if w is None else torch.from_numpy(w).double()
    if not grads:
        y = layer(g, x.to(dev), None if state is None else state.to(dev))
        ref = ref_tgcn(s, t, n, x.double(), ps, None if state is None else state.double(), loops, wt)
        close(y, ref, "TGCN forward")
        return
    xr = x.double().requires_grad_()
    pr = [None if p is None else p.clone().requires_grad_() for p in ps]
    sr = None if state is None else state.double().requires_grad_()
    ref = ref_tgcn(s, t, n, xr, pr, sr, loops, wt)
    dy = torch.from_numpy(rng.standard_normal(tuple(ref.shape)))
    ref_g = torch.autograd.grad(ref, [xr] + ([sr] if sr is not None else []) + [p for p in pr if p is not None], dy)
    xd = x.to(dev).requires_grad_()
    for p in layer.cell.parameters():
        if p is not None:
            p.requires_grad_()
    sd = None if state is None else state.to(dev).float().requires_grad_()
    y = gnnmp.tgcn_ad(layer, g, xd, sd)
    close(y, ref, "TGCN forward (tgcn_ad)")
    close(layer(g, xd.detach(), None if sd is None else sd.detach()), ref, "TGCN forward")
    got_g = torch.autograd.grad(y, [xd] + ([sd] if sd is not None else []) + [p for p in layer.cell.parameters() if p is not None],
                                dy.float().to(dev))
    names = ["x"] + (["state"] if sd is not None else []) + [f"param{k}" for k, p in enumerate(ps) if p is not None]
    for nm, a, b in zip(names, got_g, ref_g):
        close(a, b, f"grad {nm}")


CASES = {
    "reference_test_case": dict(n=4, m=8, cin=3, cout=5, T=5),
    "example_T3": dict(n=207, m=1722, cin=2, cout=100, T=3),
    "example_T12": dict(n=207, m=1722, cin=2, cout=100, T=12),
    "w_first": dict(n=30, m=120, cin=16, cout=8, T=4),
    "out1": dict(n=40, m=160, cin=3, cout=1, T=4),
    "out7": dict(n=40, m=160, cin=3, cout=7, T=4),
    "out64": dict(n=50, m=200, cin=3, cout=64, T=3),
    "out128": dict(n=50, m=200, cin=3, cout=128, T=3),
    "out_beyond_envelope": dict(n=20, m=60, cin=3, cout=136, T=2),
    "T1": dict(n=25, m=80, cin=4, cout=9, T=1),
    # backward_temporal.py's slicing (_diag_blocks, the dU blocks, stacked_params) at NT = 3, 5, 6 and the ragged NT = 8
    "out40": dict(n=40, m=160, cin=3, cout=40, T=3),
    "out72": dict(n=40, m=160, cin=3, cout=72, T=3),
    "out90": dict(n=40, m=160, cin=3, cout=90, T=3),
    "out120": dict(n=40, m=160, cin=3, cout=120, T=3),
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_tgcn_forward_and_gradients(case):
    from gnnmp import synth
    c = CASES[case]
    s1, t1 = synth.rand_graph(c["n"], c["m"], np.random.default_rng(7))
    _run_case(s1, t1, c["n"], c["cin"], c["cout"], c["T"])


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["matrix", "vector"])
def test_tgcn_with_state(kind):
    from gnnmp import synth
    s1, t1 = synth.rand_graph(4, 8, np.random.default_rng(7))
    rng = np.random.default_rng(5)
    st = torch.from_numpy(rng.standard_normal((4, 5) if kind == "matrix" else (5,)).astype(np.float32))
    _run_case(s1, t1, 4, 3, 5, 5, state=st)
    s1, t1 = synth.rand_graph(60, 300, np.random.default_rng(8))
    st = torch.from_numpy(rng.standard_normal((60, 100) if kind == "matrix" else (100,)).astype(np.float32))
    _run_case(s1, t1, 60, 2, 100, 3, state=st)


@pytest.mark.gpu
def test_tgcn_bias_false_and_no_self_loops():
    s1, t1 = road_graph(50, seed=2)        # every node has in-edges: no isolated destination
    _run_case(s1, t1, 50, 3, 12, 3, bias=False, loops=False)


@pytest.mark.gpu
def test_tgcn_edge_weights_forward():
    s1, t1 = road_graph(40, seed=3)
    w = np.random.default_rng(4).random(len(s1)).astype(np.float32) + 0.5
    _run_case(s1, t1, 40, 3, 20, 3, w=w, grads=False)
    import gnnmp
    g = gnnmp.GNNGraph(torch.from_numpy(s1).cuda(), torch.from_numpy(t1).cuda(), w=torch.from_numpy(w).cuda(), num_nodes=40)
    layer = gnnmp.TGCN((3, 20), use_edge_weight=True)
    with pytest.raises(NotImplementedError):
        gnnmp.tgcn_ad(layer, g, torch.zeros((40, 3, 3), device="cuda"))


@pytest.mark.gpu
def test_tgcn_hubs_isolated_nodes_and_ragged_tiles():
    """a hub destination with 700 in-edges (above the 512 split threshold), isolated nodes, N = 1003 (not a multiple of 16 or 64)"""
    rng = np.random.default_rng(11)
    n = 1003
    s0, t0 = road_graph(900, deg=4, seed=5)
    hub_src = rng.choice(np.arange(2, 901), 700, replace=False).astype(np.int64)
    s1 = np.concatenate([s0, hub_src])
    t1 = np.concatenate([t0, np.ones(700, np.int64)])
    _run_case(s1, t1, n, 3, 24, 3)


@pytest.mark.gpu
def test_tgcn_on_a_batch_of_road_graphs():
    import gnnmp
    members = []
    for k in range(64):
        s, t = road_graph(207, seed=100 + k)
        members.append(gnnmp.GNNGraph(torch.from_numpy(s).cuda(), torch.from_numpy(t).cuda(), num_nodes=207))
    gb = gnnmp.batch(members)
    s1 = gb.s.cpu().numpy().astype(np.int64) + (1 - gb.index_base)
    t1 = gb.t.cpu().numpy().astype(np.int64) + (1 - gb.index_base)
    _run_case(s1, t1, gb.num_nodes, 2, 32, 3, grads=True)


@pytest.mark.gpu
def test_fused_and_per_step_paths_agree_and_runs_are_bit_identical():
    import gnnmp
    from gnnmp import _lib
    s1, t1 = road_graph(207, seed=9)
    g = gnnmp.GNNGraph(torch.from_numpy(s1).cuda(), torch.from_numpy(t1).cuda(), num_nodes=207)
    layer = gnnmp.TGCN((2, 100), seed=4)
    x = torch.randn((207, 12, 2), device="cuda")
    st = torch.randn((207, 100), device="cuda")

    def run():
        xd = x.clone().requires_grad_()
        sd = st.clone().requires_grad_()
        for p in layer.cell.parameters():
            p.requires_grad_()
        y = gnnmp.tgcn_ad(layer, g, xd, sd)
        gr = torch.autograd.grad(y, [xd, sd] + layer.cell.parameters(), torch.ones_like(y))
        return [y.detach()] + list(gr)

    a, b = run(), run()
    for u, v in zip(a, b):
        assert torch.equal(u, v), "two runs differ"
    with _lib.tuned(_lib.Knob.TGCN, -1):
        c = run()
    for k, (u, v) in enumerate(zip(a, c)):
        close(u, v, f"fused vs per-step, output {k}")


@pytest.mark.gpu
def test_chain_tgcn_dense_shape_and_gradients():
    import gnnmp
    from gnnmp.backward import dense_ad
    s1, t1 = road_graph(207, seed=1)
    g = gnnmp.GNNGraph(torch.from_numpy(s1).cuda(), torch.from_numpy(t1).cuda(), num_nodes=207)
    model = gnnmp.GNNChain(gnnmp.TGCN((2, 100), seed=3), gnnmp.Dense((100, 1), seed=5))
    x = torch.randn((207, 3, 2), device="cuda")
    y = model(g, x)
    assert tuple(y.shape) == (207, 3, 1)
    tg, head = model.layers
    params = [p.requires_grad_() for p in tg.cell.parameters() + [head.weight, head.bias]]
    xd = x.clone().requires_grad_()
    y2 = dense_ad(head, gnnmp.tgcn_ad(tg, g, xd))
    close(y2.detach(), y, "chain with and without autograd")
    loss = (y2 ** 2).mean()
    gr = torch.autograd.grad(loss, [xd] + params)
    assert all(torch.isfinite(v).all() for v in gr) and float(gr[-2].abs().sum()) > 0
    # against the restatement + a float64 Dense
    ps = [p.detach().cpu().double().requires_grad_() for p in tg.cell.parameters()]
    hw, hb = head.weight.detach().cpu().double().requires_grad_(), head.bias.detach().cpu().double().requires_grad_()
    xr = x.cpu().double().requires_grad_()
    yr = ref_tgcn(torch.from_numpy(s1 - 1), torch.from_numpy(t1 - 1), 207, xr, ps) @ hw.T + hb
    rg = torch.autograd.grad((yr ** 2).mean(), [xr] + ps + [hw, hb])
    for k, (a, b) in enumerate(zip(gr, rg)):
        close(a, b, f"chain grad {k}")


@pytest.mark.gpu
def test_training_learns_a_diffusion_signal():
    """GNNChain(TGCN(1 => 32), Dense(32 => 1)) learns to predict, for each of 4 steps, the one-hop mean of a seeded random signal over a
    road-like graph (a diffusion step).  Adam (lr 0.01), 150 full-batch steps, fixed seeds.  Bar: the final loss ends below 70 % of the
    initial loss.  A model that does not learn stays near 100 %; the float64 restatement trained the same way ends at 55 %."""
    import gnnmp
    from gnnmp.backward import dense_ad
    torch.manual_seed(0)
    n, T = 207, 4
    s1, t1 = road_graph(n, seed=21)
    g = gnnmp.GNNGraph(torch.from_numpy(s1).cuda(), torch.from_numpy(t1).cuda(), num_nodes=n)
    st, tt = torch.from_numpy(s1 - 1), torch.from_numpy(t1 - 1)
    deg = torch.zeros(n).index_add(0, tt, torch.ones(len(tt)))
    gen = torch.Generator().manual_seed(1)
    x = torch.randn((n, T, 1), generator=gen)
    target = torch.zeros_like(x)
    for k in range(T):
        target[:, k] = torch.zeros((n, 1)).index_add(0, tt, x[st, k]) / deg[:, None]
    x, target = x.cuda(), target.cuda()
    tg, head = gnnmp.TGCN((1, 32), seed=7), gnnmp.Dense((32, 1), seed=8)
    params = [p.requires_grad_() for p in tg.cell.parameters() + [head.weight, head.bias]]
    opt = torch.optim.Adam(params, lr=0.01)
    losses = []
    for _ in range(150):
        loss = ((dense_ad(head, gnnmp.tgcn_ad(tg, g, x)) - target) ** 2).mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(loss.item())
    assert losses[-1] < 0.7 * losses[0], losses[::15]
