"""TopKPool on the device (csrc/topk.hip, gnnmp_plan_keep_nodes, gnnmp/pool_topk.py) against tests/topk_ref.py.
The selection is compared WITHOUT a tolerance, always on the fp32 scores the device itself holds (read back), never on a float64 score;
values (scores, gated features, gradients) owe the project's bar: 1e-5, norm-wise and element-wise against the reference's scale."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import topk_ref as R  # noqa: E402

gpu = pytest.mark.gpu
RTOL = 1e-5
DEV_FROM_12 = 4 * 11          # lds_budget_bytes that holds 11 keys: member graphs of 12 nodes and more take the device-memory route
KS = ((1, 0.0), (4, 0.0), (64, 0.0), (2000, 0.0), (0, 0.1), (0, 0.5), (0, 1.0))      # (k, ratio): 2000 keeps all
CS = (1, 3, 7, 64, 100, 129, 513)


@pytest.fixture(scope="module")
def gm():
    import torch
    assert torch.cuda.is_available()
    import gnnmp
    gnnmp.load()
    return gnnmp


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.detach().cpu().numpy()


def close(got, ref, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, what
    if ref.size == 0:
        return
    assert np.all(np.isfinite(got)), what
    assert np.linalg.norm(got - ref) <= RTOL * np.linalg.norm(ref), f"{what}: norm-wise"
    worst = np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-30)
    assert worst <= RTOL, f"{what}: element-wise, {worst:.2e} of the reference's scale"


def _select(y, ptr, ib, k, ratio, ties, budget):
    """gnnmp_topk_select_f32 through ctypes: (keep uint32 [N + 1], rank int32 [N]) as numpy; the outputs start poisoned"""
    import torch
    from gnnmp import _lib as L
    N = y.numel()
    keep = torch.full((N + 1,), -7, dtype=torch.int32, device="cuda")
    rank = torch.full((N,), -7, dtype=torch.int32, device="cuda")
    job = L.TopkJob(L.ptr(y), L.ptr(ptr), ib, 1 if ptr is None else ptr.numel() - 1, k, ratio, ties, budget, L.ptr(keep), L.ptr(rank))
    L.check(L.load().gnnmp_topk_select_f32(ctypes.byref(job), N, L.stream_ptr()))
    return _np(keep).view(np.uint32), _np(rank)


# ---- selection, exact -----------------------------------------------------------------------------------------------------------------
VECTORS = ("random", "equal", "tie_block", "negative", "specials", "descending", "ascending", "device_y")


@gpu
@pytest.mark.parametrize("name", VECTORS)
def test_selection_is_the_restatement_bit_for_bit(gm, name):
    from gnnmp.pool_topk import topk_score
    ptr = R.batch_ptr()
    N = int(ptr[-1])
    if name == "device_y":                                   # scores the device's own projection made
        rng = np.random.default_rng(5)
        y = topk_score(_dev(rng.standard_normal((N, 7)).astype(np.float32)), _dev(rng.standard_normal(7).astype(np.float32)))
    else:
        y = _dev(R.score_vectors(ptr)[name])
    y_back = _np(y)                                          # the restatement is applied to the device's own scores, read back
    ptrs = {8: _dev(ptr), 4: _dev(ptr.astype(np.int32))}
    n = 0
    for k, ratio in KS:
        for ties in (R.FIRST, R.ALL):
            keep_ref, rank_ref = R.select(y_back, ptr, k, ratio, ties)
            one_ref = R.select(y_back, None, k, ratio, ties)
            for budget in (0, DEV_FROM_12):
                for ib in (4, 8):
                    keep, rank = _select(y, ptrs[ib], ib, k, ratio, ties, budget)
                    tag = f"{name} k{k} r{ratio} ties{ties} budget{budget} ib{ib}"
                    assert np.array_equal(keep, keep_ref), tag
                    assert np.array_equal(rank, rank_ref), tag
                    n += 1
            for budget in (0, DEV_FROM_12, 64 * 1024):       # graph_ptr = NULL: one graph of 1993 nodes, on either route
                keep, rank = _select(y, None, 8, k, ratio, ties, budget)
                assert np.array_equal(keep, one_ref[0]) and np.array_equal(rank, one_ref[1]), f"{name} k{k} r{ratio} ties{ties} one graph, budget {budget}"
    assert n == 56


@gpu
def test_selection_of_small_shapes(gm):
    """no node; one node; a batch of empty graphs only; the reference's known answer"""
    import torch
    keep, rank = _select(torch.zeros(0, device="cuda"), None, 8, 3, 0.0, R.FIRST, 0)
    assert keep.tolist() == [0] and rank.size == 0
    keep, rank = _select(_dev(np.array([np.nan], np.float32)), None, 8, 1, 0.0, R.ALL, 0)
    assert keep.tolist() == [1, 0] and rank.tolist() == [0]
    keep, _ = _select(torch.zeros(0, device="cuda"), _dev(np.zeros(4, np.int64)), 8, 0, 0.5, R.FIRST, 0)
    assert keep.tolist() == [0]
    y = _dev(np.array([8, 7, 6, 5, 4, 3, 2, 1], np.float32))
    assert _np(gm.topk_index(y, 4)).tolist() == [1, 2, 3, 4] and _np(gm.topk_index(y.reshape(1, 8), 4)).tolist() == [1, 2, 3, 4]
    t = _dev(np.array([3, 5, 5, 5, 1], np.float32))
    assert _np(gm.topk_index(t, 2)).tolist() == [2, 3, 4] and _np(gm.topk_index(t, 2, ties="first")).tolist() == [2, 3]
    g = gm.GNNGraph([1, 4], [2, 5], num_nodes=5, graph_indicator=[1, 1, 1, 2, 2], num_graphs=2, index_base=1)
    assert _np(gm.topk_index(t, 1, g)).tolist() == [2, 3, 4] and _np(gm.topk_index(t, 1, g, ties="first")).tolist() == [2, 4]      # per member graph


# ---- score and gate -------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("C", CS)
def test_score_and_gate_against_float64(gm, C):
    from gnnmp import pool_topk as PT
    rng = np.random.default_rng(100 + C)
    ptr = np.array([0, 40, 41, 41, 170, 300])
    N = int(ptr[-1])
    x, p = rng.standard_normal((N, C)).astype(np.float32), rng.standard_normal(C).astype(np.float32)
    xd, pd = _dev(x), _dev(p)
    y = PT.topk_score(xd, pd)
    y64 = R.score64(x, p)
    close(_np(y), y64, f"y at C = {C}")
    gi = np.repeat(np.arange(1, 6), np.diff(ptr))
    g = gm.GNNGraph(np.array([1, 2], np.int64), np.array([2, 1], np.int64), num_nodes=N, graph_indicator=gi, num_graphs=5)
    keep, _ = PT.topk_select(y, 0, 0.5, g, "first")
    idx0 = np.flatnonzero(_np(keep)[:-1])                    # the device's own selection
    assert np.array_equal(_np(keep).view(np.uint32), R.select(_np(y), ptr, 0, 0.5, R.FIRST)[0])
    for act, code in R.ACTS.items():
        x2 = PT._gate(xd, y, _dev(idx0.astype(np.int32)), act)
        close(_np(x2), R.gate64(x, y64, idx0, code), f"x2 at C = {C}, {act}")


# ---- end to end, exact inputs ---------------------------------------------------------------------------------------------------------
def _exact_batch(gm, seed=11, sizes=(9, 1, 14, 6), weights=True):
    """a batch whose scores are exact in fp32 and float64 alike and contain ties: x small integers, p = (1, 1, 1, 1, 0, 0, 0)"""
    rng = np.random.default_rng(seed)
    ptr = np.concatenate([[0], np.cumsum(sizes)])
    N = int(ptr[-1])
    s0 = np.concatenate([a + rng.integers(0, n, 3 * n) for a, n in zip(ptr[:-1], sizes)])
    t0 = np.concatenate([a + rng.integers(0, n, 3 * n) for a, n in zip(ptr[:-1], sizes)])
    x = rng.integers(-2, 3, (N, 7)).astype(np.float32)
    w = rng.random(len(s0)).astype(np.float32) if weights else None
    gi = np.repeat(np.arange(1, len(sizes) + 1), sizes)
    g = gm.GNNGraph(_dev(s0 + 1), _dev(t0 + 1), None if w is None else _dev(w), num_nodes=N, graph_indicator=_dev(gi), num_graphs=len(sizes),
                    x=_dev(x))
    return g, dict(s0=s0, t0=t0, x=x, w=w, gi=gi, ptr=ptr, N=N)


@gpu
@pytest.mark.parametrize("k, act", [(3, "sigmoid"), (0.5, "tanh"), (1, "identity"), (40, "sigmoid")])
def test_layer_end_to_end_against_the_restatement(gm, k, act):
    import torch
    import test_plan_edit as PE
    g, h = _exact_batch(gm)
    p = np.array([1, 1, 1, 1, 0, 0, 0], np.float32)
    y64 = R.score64(h["x"], p)
    assert np.array_equal(y64, h["x"][:, :4].sum(1) / 2.0) and np.array_equal(y64.astype(np.float32).astype(np.float64), y64)      # exact
    assert any(len(np.unique(y64[a:b])) < b - a for a, b in zip(h["ptr"][:-1], h["ptr"][1:]))                                        # ties
    l = gm.TopKPool(k, 7, act=act)
    l.p = _dev(p)
    kk, ratio = (k, 0.0) if isinstance(k, int) else (0, k)
    idx0, x2_ref, s2, t2, eid = R.topk_pool(h["x"], p, h["s0"], h["t0"], h["ptr"], kk, ratio, R.ACTS[act])
    g2, x2 = l(g, g.x)
    assert isinstance(g2, gm.GNNGraph) and (g2.num_nodes, g2.num_edges, g2.num_graphs) == (len(idx0), len(s2), 4)
    assert np.array_equal(_np(g2.nid), idx0 + 1) and np.array_equal(_np(g2.eid), eid + 1) and g2.nid.dtype == g.s.dtype
    assert np.array_equal(_np(g2.s), s2 + 1) and np.array_equal(_np(g2.t), t2 + 1)
    close(_np(x2), x2_ref, "x2")
    # the indicator, the weights and g.x follow as in a remove_nodes of the complementary list
    drop = np.setdiff1d(np.arange(h["N"]), idx0)
    twin = gm.remove_nodes(g, (drop + 1).tolist())
    for a, b in ((g2.graph_indicator, twin.graph_indicator), (g2.w, twin.w), (g2.x, twin.x), (g2.nid, twin.nid), (g2.eid, twin.eid)):
        assert torch.equal(a, b)
    ed = {"e": torch.arange(g.num_edges, device="cuda", dtype=torch.float32).reshape(-1, 1)}
    _, _, ed2 = gm.topk_pool(l, g, g.x, edata=ed)
    assert np.array_equal(_np(ed2["e"]).reshape(-1), eid.astype(np.float32))
    # plan(), the self-looped and the transposed plans: derived from the parent's cached ones, bit-identical to plans built from g2's edges
    PE._derived_equals_built(gm, g, lambda: l(g, g.x)[0])
    # the reference's positional form: the layer holds the graph
    held = gm.TopKPool(g, k, 7, act=act)
    held.p = l.p
    assert torch.equal(held(g.x)[1], x2)
    # an externally supplied score (SAGPool): the projection is skipped
    ys = _dev(y64.astype(np.float32)[::-1].copy())
    g3, x3 = l(g, g.x, score=ys)
    keep3 = R.select(_np(ys), h["ptr"], kk, ratio, R.FIRST)[0][:-1].astype(bool)
    assert np.array_equal(_np(g3.nid), np.flatnonzero(keep3) + 1)
    close(_np(x3), R.gate64(h["x"], _np(ys), np.flatnonzero(keep3), R.ACTS[act]), "x2 with a given score")


# ---- gnnmp_plan_keep_nodes ------------------------------------------------------------------------------------------------------------
def _keep_plan(parent, mask):
    import torch
    from gnnmp import _lib as L
    from gnnmp.graph import Plan
    N, E = parent.n_dst, parent.n_edges
    h, tot = ctypes.c_void_p(), (ctypes.c_int64 * 2)()
    nm = torch.full((max(N, 1),), -7, dtype=torch.int32, device="cuda")
    nn = torch.full((max(N, 1),), -7, dtype=torch.int32, device="cuda")
    em = torch.full((max(E, 1),), -7, dtype=torch.int32, device="cuda")
    L.check(L.load().gnnmp_plan_keep_nodes(ctypes.byref(h), parent.handle, L.ptr(mask), L.ptr(nm), L.ptr(nn), L.ptr(em), tot, L.stream_ptr()))
    return Plan._adopt(h, parent.device), tot[0], tot[1], _np(nm), _np(nn)[:N], _np(em)


@gpu
@pytest.mark.parametrize("name", ["n33_e0", "n300_e300", "n4097_e4097", "hub", "n0"])
def test_plan_keep_nodes_is_plan_remove_nodes_with_the_mask_supplied(gm, name):
    import torch
    import test_plan_edit as PE
    s0, t0, N = PE.GRAPHS[name] if name != "n0" else (np.zeros(0, np.int64), np.zeros(0, np.int64), 0)
    rng = np.random.default_rng(N + 1)
    pick = rng.choice(N, max(1, N // 3), replace=False) if N else np.zeros(0, np.int64)
    lists = {"list": pick, "ones": np.zeros(0, np.int64), "zeros": np.arange(N)}
    for loops, tr in PE.KINDS:
        parent = PE._plan(s0, t0, N, 0, 8, loops, tr)
        for what, lst in lists.items():
            mask = np.full(N, 0x80000001, np.uint32)                   # any non-zero word keeps
            mask[lst] = 0
            mt = _dev(mask.view(np.int32)) if N else None
            nm_r = torch.full((max(N, 1),), -7, dtype=torch.int32, device="cuda")
            nn_r = torch.full((max(N, 1),), -7, dtype=torch.int32, device="cuda")
            em_r = torch.full((max(len(s0), 1),), -7, dtype=torch.int32, device="cuda")
            ref, nk_r, ek_r = PE._remove(parent, _dev(lst) if len(lst) else None, 8, 0, maps=(nm_r, nn_r, em_r))
            child, nk, ek, nm, nn, em = _keep_plan(parent, mt)
            tag = f"{name} {what} loops{loops} T{tr}"
            assert (nk, ek) == (nk_r, ek_r) == (N - len(lst), ek_r), tag
            PE._same(child, ref, tag)
            assert np.array_equal(nm, _np(nm_r)) and np.array_equal(nn, _np(nn_r)[:N]) and np.array_equal(em, _np(em_r)), tag


# ---- the pullback -----------------------------------------------------------------------------------------------------------------------
def _act_t(act, y):
    import torch
    return torch.sigmoid(y) if act == "sigmoid" else torch.tanh(y) if act == "tanh" else y


def _batch_graph(gm, sizes):
    ptr = R.batch_ptr(sizes)
    N = int(ptr[-1])
    gi = np.repeat(np.arange(1, len(sizes) + 1), sizes)
    e = np.arange(1, max(N, 2), dtype=np.int64)                              # a path (inside and across members: the gate ignores edges)
    e = e[e < N] if N > 1 else np.zeros(0, np.int64)
    return gm.GNNGraph(_dev(e), _dev(e + 1), num_nodes=N, graph_indicator=_dev(gi), num_graphs=len(sizes)), N


@gpu
@pytest.mark.parametrize("sizes, C, act", [(R.SIZES, 7, "sigmoid"), (R.SIZES, 64, "tanh"), (R.SIZES, 7, "identity"), ((1,), 7, "sigmoid")])
def test_pullback_against_float64_autograd(gm, sizes, C, act):
    import torch
    g, N = _batch_graph(gm, sizes)
    rng = np.random.default_rng(C + len(sizes))
    x, p = rng.standard_normal((N, C)).astype(np.float32), rng.standard_normal(C).astype(np.float32)
    l = gm.TopKPool(0.5, C, act=act)

    def device(score=None):
        xt = _dev(x).requires_grad_(True)
        l.p = _dev(p).requires_grad_(True)
        st = None if score is None else _dev(score).requires_grad_(True)
        g2, x2 = gm.topk_pool_ad(l, g, xt, score=st)
        assert not g2.nid.requires_grad
        W = _dev(np.random.default_rng(9).standard_normal(tuple(x2.shape)).astype(np.float32))
        x2.backward(W)
        return _np(g2.nid) - 1, _np(x2), _np(W), _np(xt.grad), (None if score is not None else _np(l.p.grad)), (None if st is None else _np(st.grad))

    # differentiable in x and p
    idx0, x2, W, dx, dp, _ = device()
    xr, pr = torch.from_numpy(x).double().requires_grad_(True), torch.from_numpy(p).double().requires_grad_(True)
    yr = xr @ pr / pr.norm()
    x2r = xr[idx0] * _act_t(act, yr[idx0])[:, None]                          # the device's selection, held fixed
    (x2r * torch.from_numpy(W).double()).sum().backward()
    close(x2, x2r.detach().numpy(), "x2")
    close(dx, xr.grad.numpy(), "dx")
    close(dp, pr.grad.numpy(), "dp")
    dropped = np.setdiff1d(np.arange(N), idx0)
    assert len(dropped) > 0 or N == 1
    assert not dx[dropped].any() and not np.signbit(dx[dropped]).any(), "dx rows of dropped nodes are exactly zero"
    again = device()
    assert np.array_equal(again[3].view(np.uint32), dx.view(np.uint32)) and np.array_equal(again[4].view(np.uint32), dp.view(np.uint32))
    # differentiable in x and an externally supplied score
    score = rng.standard_normal(N).astype(np.float32)
    idx0, x2, W, dx, _, dy = device(score)
    xr, sr = torch.from_numpy(x).double().requires_grad_(True), torch.from_numpy(score).double().requires_grad_(True)
    x2r = xr[idx0] * _act_t(act, sr[idx0])[:, None]
    (x2r * torch.from_numpy(W).double()).sum().backward()
    close(x2, x2r.detach().numpy(), "x2 (score)")
    close(dx, xr.grad.numpy(), "dx (score)")
    close(dy, sr.grad.numpy(), "dy")
    dropped = np.setdiff1d(np.arange(N), idx0)
    assert not dx[dropped].any() and not dy[dropped].any()
    assert np.array_equal(device(score)[5].view(np.uint32), dy.view(np.uint32))


# ---- a training step ----------------------------------------------------------------------------------------------------------------------
def _gcn64(A, x, W, b):
    """GCNConv in float64 on the dense A[t, s] (edge counts): relu(Â x W' + b), Â = D^-1/2 (A + I) D^-1/2 with D the in-degrees of A + I"""
    import torch
    At = A + torch.eye(A.shape[0], dtype=torch.float64)
    c = At.sum(1).rsqrt()
    return torch.relu((c[:, None] * At * c[None, :]) @ x @ W.T + b)


@gpu
def test_training_step_conv_pool_conv_readout(gm):
    import torch
    from gnnmp.backward import gcn_conv_ad, global_pool_ad
    rng = np.random.default_rng(21)
    G, n, D = 5, 10, 7
    N = G * n
    u = np.concatenate([a * n + rng.integers(0, n, 15) for a in range(G)])
    v = np.concatenate([a * n + rng.integers(0, n, 15) for a in range(G)])
    ok = u != v
    s0, t0 = np.concatenate([u[ok], v[ok]]), np.concatenate([v[ok], u[ok]])      # both directions: in-degree = out-degree
    gi = np.repeat(np.arange(1, G + 1), n)
    g = gm.GNNGraph(_dev(s0 + 1), _dev(t0 + 1), num_nodes=N, graph_indicator=_dev(gi), num_graphs=G)
    x = rng.standard_normal((N, D)).astype(np.float32)
    c1, c2 = gm.GCNConv((D, 8), "relu", seed=1), gm.GCNConv((8, 6), "relu", seed=2)
    pool, read = gm.TopKPool(4, 8, seed=3), gm.GlobalPool("mean")
    params = [c1.weight, c1.bias, pool.p, c2.weight, c2.bias]
    for t in params:
        t.requires_grad_(True)
    xt = _dev(x).requires_grad_(True)
    h1 = gcn_conv_ad(c1, g, xt)
    g2, h2 = gm.topk_pool_ad(pool, g, h1)
    out = global_pool_ad(read, g2, gcn_conv_ad(c2, g2, h2))
    assert tuple(out.shape) == (G, 6) and g2.num_nodes == 4 * G and g2.num_graphs == G
    Wout = _dev(rng.standard_normal((G, 6)).astype(np.float32))
    out.backward(Wout)
    grads = [_np(xt.grad)] + [_np(t.grad) for t in params]
    assert all(np.all(np.isfinite(gr)) for gr in grads)

    # float64, with the device's selection held fixed
    idx0 = _np(g2.nid) - 1
    A = torch.zeros((N, N), dtype=torch.float64)
    A.index_put_((torch.from_numpy(t0), torch.from_numpy(s0)), torch.ones(len(s0), dtype=torch.float64), accumulate=True)
    xr = torch.from_numpy(x).double().requires_grad_(True)
    pr = [t.detach().cpu().double().requires_grad_(True) for t in params]
    h1r = _gcn64(A, xr, pr[0], pr[1])
    yr = h1r @ pr[2] / pr[2].norm()
    h2r = h1r[idx0] * torch.sigmoid(yr[idx0])[:, None]
    h3r = _gcn64(A[idx0][:, idx0], h2r, pr[3], pr[4])
    outr = h3r.reshape(G, 4, 6).mean(1)                                           # (the kept nodes ascend: four a member graph)
    assert np.array_equal(gi[idx0], np.repeat(np.arange(1, G + 1), 4))
    (outr * Wout.cpu().double()).sum().backward()
    close(_np(out), outr.detach().numpy(), "the model's output")
    for name, got, ref in zip(("dx", "dW1", "db1", "dp", "dW2", "db2"), grads, [xr.grad] + [t.grad for t in pr]):
        close(got, ref.numpy(), name)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
@gpu
def test_refusals_by_name_with_nothing_written(gm):
    import torch
    g, h = _exact_batch(gm)
    l = gm.TopKPool(3, 7)
    x = g.x

    class Hetero:
        is_hetero = True
    sp = gm.GNNGraph.from_sparse(colptr=torch.tensor([1, 2, 3, 3]), rowval=torch.tensor([2, 1]))
    tg = object.__new__(gm.TemporalSnapshotsGNNGraph)
    for fn in (gm.topk_pool, gm.topk_pool_ad):
        with pytest.raises(TypeError, match="GNNHeteroGraph is not supported"):
            fn(l, Hetero(), x)
        with pytest.raises(TypeError, match="TemporalSnapshotsGNNGraph is not supported"):
            fn(l, tg, x)
        with pytest.raises(TypeError, match="sparse-matrix graphs"):
            fn(l, sp, x[:3])
        with pytest.raises(ValueError, match="x has shape"):
            fn(l, g, x[:-1])
        with pytest.raises(ValueError, match="channels"):
            fn(l, g, x[:, :5].contiguous())
        with pytest.raises(ValueError, match="scores for the"):
            fn(l, g, x, score=torch.zeros(h["N"] + 1, device="cuda"))
    for bad in (np.ones((4, 4), np.float32), torch.ones(4, 4), [[0, 1], [1, 0]]):
        with pytest.raises(TypeError, match="dense adjacency matrix is not supported.*GNNGraph"):
            gm.TopKPool(bad, 2, 7)
    with pytest.raises(TypeError, match="sparse-matrix graphs"):
        gm.TopKPool(sp, 2, 7)
    for bad in (0, -3):
        with pytest.raises(ValueError, match="at least 1"):
            gm.TopKPool(bad, 7)
        with pytest.raises(ValueError, match="at least 1"):
            gm.topk_index(x[:, 0].contiguous(), bad)
    for bad in (0.0, -0.5, 1.5, float("nan")):
        with pytest.raises(ValueError, match=r"outside \(0, 1\]"):
            gm.TopKPool(bad, 7)
    with pytest.raises(ValueError, match="act"):
        gm.TopKPool(2, 7, act="relu")
    with pytest.raises(ValueError, match="values for the"):
        gm.topk_index(x[:5, 0].contiguous(), 2, g)
    # the C ABI: a refused call leaves its outputs as they were
    from gnnmp import _lib as L
    keep = torch.full((h["N"] + 1,), -7, dtype=torch.int32, device="cuda")
    y = torch.zeros(h["N"], device="cuda")
    for k, ratio, ties in ((-1, 0.0, 0), (0, 0.0, 0), (0, 1.5, 0), (2, 0.0, 5)):
        job = L.TopkJob(L.ptr(y), None, 8, 1, k, ratio, ties, 0, L.ptr(keep), None)
        assert L.load().gnnmp_topk_select_f32(ctypes.byref(job), h["N"], L.stream_ptr()) == L.EINVAL
    torch.cuda.synchronize()
    assert bool((keep == -7).all())
