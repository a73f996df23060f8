"""rand_temporal_radius_graph / rand_temporal_hyperbolic_graph (gnnmp/generate.py; GNNGraphs/src/generate.jl:265-380).

Without a GPU: the pure trajectory functions on CPU tensors against the float64 restatement of tests/temporal_gen_ref.py under the same
draws, 1e-12 relative, with draws that force a bounce off each wall and both reflections of the quantile.

On the GPU: the fields; every snapshot equal — edge list and plan bits — to radius_graph / hyperbolic_graph on that snapshot's returned
positions alone; tg.batched() already there after ONE search and equal to gnnmp.batch(tg.snapshots); dir = :out; seeds; the reference's
known answers (its docstring's complete graph, its test file's monotone mean degree); EvolveGCNO over a generated temporal graph
against the same layer over the same snapshots built one by one."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import temporal_gen_ref as R  # noqa: E402

gpu = pytest.mark.gpu


def _rel(got, ref):
    return float(np.max(np.abs(got - ref) / np.maximum(np.abs(ref), 1e-300))) if ref.size else 0.0


# ---- without a GPU: the trajectories -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,N,speed", [(6, 40, 0.3), (4, 1, 0.9), (1, 5, 0.1)])
def test_radius_trajectory_against_float64(T, N, speed):
    import torch
    from gnnmp import generate as G
    rng = np.random.default_rng(10 * T + N)
    u0, ur, ut = rng.random((N, 2)), rng.random((T - 1, N)), rng.random((T - 1, N))
    ref = R.radius_trajectory(u0, ur, ut, speed)
    args = [torch.from_numpy(a) for a in (u0, ur, ut)]
    got64 = G.radius_trajectory(*args, speed, dtype=torch.float64).numpy()
    assert got64.shape == (T, N, 2) and _rel(got64, ref) <= 1e-12
    got = G.radius_trajectory(*args, speed)
    assert got.dtype == torch.float32 and np.array_equal(got.numpy(), got64.astype(np.float32))      # rounded once, at the end
    assert got64.min() >= 0.0 and got64.max() <= 1.0


def test_radius_trajectory_bounces_off_each_wall():
    import torch
    from gnnmp import generate as G
    speed = 0.2
    u0 = np.array([[0.02, 0.5], [0.95, 0.5], [0.5, 0.95], [0.5, 0.02]])
    ur = np.full((1, 4), 0.999)                                   # rho = +0.1996
    ut = np.array([[0.5, 0.0, 0.25, 0.75]])                       # theta = pi, 0, pi / 2, 3 pi / 2: towards x = 0, x = 1, y = 1, y = 0
    rho = 2 * speed * 0.999 - speed
    raw = [0.02 - rho, 0.95 + rho, 0.95 + rho, 0.02 - rho]
    assert raw[0] < 0 < 1 < raw[1] and raw[2] > 1 and raw[3] < 0
    got = G.radius_trajectory(*[torch.from_numpy(a) for a in (u0, ur, ut)], speed, dtype=torch.float64).numpy()
    ref = R.radius_trajectory(u0, ur, ut, speed)
    assert _rel(got, ref) <= 1e-12
    want = [rho - 0.02, 2.0 - (0.95 + rho), 2.0 - (0.95 + rho), rho - 0.02]
    hit = [got[1, 0, 0], got[1, 1, 0], got[1, 2, 1], got[1, 3, 1]]
    assert np.allclose(hit, want, rtol=0, atol=1e-12) and got.min() >= 0.0 and got.max() <= 1.0


@pytest.mark.parametrize("T,N,alpha,Rr,speed", [(6, 40, 1.0, 4.0, 0.3), (5, 1, 0.5, 10.0, 0.8), (2, 7, 2.0, 1.0, 0.05)])
def test_hyperbolic_trajectory_against_float64(T, N, alpha, Rr, speed):
    import torch
    from gnnmp import generate as G
    rng = np.random.default_rng(T + N)
    up, uth, udp, udth = rng.random(N), rng.random(N), rng.random((T - 1, N)), rng.random((T - 1, N))
    ref, pref = R.hyperbolic_trajectory(up, uth, udp, udth, alpha, Rr, speed)
    args = [torch.from_numpy(a) for a in (up, uth, udp, udth)]
    got64, p = G.hyperbolic_trajectory(*args, alpha, Rr, speed, return_p=True, dtype=torch.float64)
    assert tuple(got64.shape) == (T, N, 2) and _rel(got64.numpy(), ref) <= 1e-12 and _rel(p.numpy(), pref) <= 1e-12
    assert p.min() >= 0.0 and p.max() <= 1.0
    assert got64[..., 0].min() >= 0.0 and got64[..., 0].max() <= Rr * (1 + 1e-12)
    got = G.hyperbolic_trajectory(*args, alpha, Rr, speed)
    assert got.dtype == torch.float32 and np.array_equal(got.numpy(), got64.numpy().astype(np.float32))


def test_hyperbolic_trajectory_reflects_the_quantile_at_both_ends():
    import torch
    from gnnmp import generate as G
    speed = 0.1
    up, uth = np.array([0.95, 0.03, 0.5]), np.array([0.0, 0.999, 0.5])
    udp = np.array([[0.95, 0.05, 0.5]])                           # steps +0.09, -0.09, 0
    udth = np.array([[0.0, 0.999, 0.5]])                          # theta drifts below 0 and above 2 pi: never wrapped
    ref, pref = R.hyperbolic_trajectory(up, uth, udp, udth, 1.0, 4.0, speed)
    got, p = G.hyperbolic_trajectory(*[torch.from_numpy(a) for a in (up, uth, udp, udth)], 1.0, 4.0, speed, return_p=True,
                                     dtype=torch.float64)
    assert _rel(got.numpy(), ref) <= 1e-12 and _rel(p.numpy(), pref) <= 1e-12
    assert np.allclose(p[1].numpy(), [1.0 - 0.04, 0.06, 0.5], rtol=0, atol=1e-12)      # 1.04 -> 1 - 0.04; -0.06 -> 0.06
    assert got[1, 0, 1] < 0.0 and got[1, 1, 1] > 2.0 * math.pi


# ---- on the GPU ----------------------------------------------------------------------------------------------------------------------------
def _same_graph(a, b):
    import torch
    return (a.num_nodes == b.num_nodes and a.num_edges == b.num_edges and torch.equal(a.s, b.s) and torch.equal(a.t, b.t)
            and (a.w is None) == (b.w is None) and (a.w is None or torch.equal(a.w, b.w)))


def _same_plan(p, q):
    import torch
    return all(torch.equal(a, b) for a, b in zip(p.export(), q.export()))


def _check_temporal(tg, pts, single, key, searches, T, N):
    """the common items: fields, every snapshot against the single-snapshot constructor, the batched form against gnnmp.batch"""
    import gnnmp
    import torch
    assert isinstance(tg, gnnmp.TemporalSnapshotsGNNGraph) and tg.num_snapshots == T and tg.num_nodes == [N] * T
    assert pts.dtype == torch.float32 and tuple(pts.shape) == (T, N, 2)
    assert searches == [T * N], "ONE search over the whole [T N, 2] batch"
    for t in range(T):
        one = single(pts[t])
        assert tg.num_edges[t] == one.num_edges and _same_graph(tg[t], one), f"snapshot {t}"
        assert key in tg[t]._plans and _same_plan(tg[t]._plans[key], one._plans[key]), f"the plan of snapshot {t}"
    assert tg._batched is not None                                   # kept from the search: batched() costs nothing
    gb, seg = tg.batched()
    assert searches == [T * N] and seg == [t * N for t in range(T + 1)]
    ref = gnnmp.batch(tg.snapshots)
    assert _same_graph(gb, ref) and gb.num_graphs == ref.num_graphs == T and torch.equal(gb.graph_indicator, ref.graph_indicator)
    assert _same_plan(gb._plans[key], ref.plan(False) if key is False else ref.plan_transposed())
    tg[0] = tg[1]
    assert tg._batched is None                                       # tg[t] = g still drops it


def _count_searches(monkeypatch, name):
    from gnnmp import generate as G
    calls, real = [], getattr(G, name)

    def counted(points, *a, **k):
        calls.append(int(points.shape[0]))
        return real(points, *a, **k)
    monkeypatch.setattr(G, name, counted)
    return calls


@gpu
@pytest.mark.parametrize("dir,loops,base,ib", [("in", False, 1, 8), ("out", True, 0, 4), ("out", False, 1, 8)])
def test_radius_generator_snapshots_and_batch(monkeypatch, dir, loops, base, ib):
    import gnnmp
    import torch
    dt = torch.int64 if ib == 8 else torch.int32
    T, N, r = 5, 37, 0.25
    searches = _count_searches(monkeypatch, "radius_graph")
    tg, pts = gnnmp.rand_temporal_radius_graph(N, T, 0.1, r, self_loops=loops, dir=dir, seed=4, return_points=True, index_base=base,
                                               idx_dtype=dt)
    assert float(pts.min()) >= 0.0 and float(pts.max()) <= 1.0 and not torch.equal(pts[0], pts[1])
    single = lambda p: gnnmp.radius_graph(p, r, self_loops=loops, dir=dir, index_base=base, idx_dtype=dt)
    assert sum(tg.num_edges) > T * N * loops
    _check_temporal(tg, pts, single, False if dir == "in" else ("T", False), searches, T, N)


@gpu
@pytest.mark.parametrize("loops,base,ib,zeta,Rr", [(False, 1, 8, 1.0, 4.0), (True, 0, 4, 0.7, 10.0)])
def test_hyperbolic_generator_snapshots_and_batch(monkeypatch, loops, base, ib, zeta, Rr):
    import gnnmp
    import torch
    dt = torch.int64 if ib == 8 else torch.int32
    T, N = 5, 37
    searches = _count_searches(monkeypatch, "hyperbolic_graph")
    tg, pts = gnnmp.rand_temporal_hyperbolic_graph(N, T, 1.0, Rr, 0.1, zeta=zeta, self_loop=loops, seed=9, return_points=True,
                                                   index_base=base, idx_dtype=dt)
    assert float(pts[..., 0].min()) >= 0.0 and float(pts[..., 0].max()) <= Rr * (1 + 1e-6)
    single = lambda p: gnnmp.hyperbolic_graph(p, Rr, zeta, self_loops=loops, index_base=base, idx_dtype=dt)
    assert all(g.w is not None and bool((g.w == 1).all()) for g in tg) and sum(tg.num_edges) > T * N * loops
    _check_temporal(tg, pts, single, False, searches, T, N)


@gpu
def test_seeds():
    import gnnmp
    import torch
    for make in (lambda s: gnnmp.rand_temporal_radius_graph(50, 4, 0.1, 0.3, seed=s, return_points=True),
                 lambda s: gnnmp.rand_temporal_hyperbolic_graph(50, 4, 1.0, 4.0, 0.1, seed=s, return_points=True)):
        (a, pa), (b, pb), (c, pc) = make(3), make(3), make(4)
        assert torch.equal(pa, pb) and a == b and all(_same_graph(x, y) for x, y in zip(a, b))
        assert not torch.equal(pa, pc) and a != c
        d = make(None)[0]
        assert d.num_snapshots == 4


@gpu
def test_known_answers_of_the_reference():
    import gnnmp
    tg = gnnmp.rand_temporal_radius_graph(10, 5, 0.1, 1.5, seed=1)       # the docstring's example: r = 1.5 covers the unit square
    assert tg.num_nodes == [10] * 5 and tg.num_edges == [90] * 5 and tg.num_snapshots == 5
    # GNNGraphs/test/generate.jl: the mean degree grows with r ...
    n, T = 30, 5
    deg = [sum(gnnmp.rand_temporal_radius_graph(n, T, 0.1, r, seed=2).num_edges) / (n * T) for r in (0.1, 0.3, 0.6, 1.5)]
    assert all(a <= b for a, b in zip(deg, deg[1:])) and deg[0] < deg[-1] == n - 1
    # ... and falls from R = 1 to R = 10 in the hyperbolic disk
    d1 = sum(gnnmp.rand_temporal_hyperbolic_graph(n, T, 1.0, 1.0, 0.1, seed=2).num_edges) / (n * T)
    d10 = sum(gnnmp.rand_temporal_hyperbolic_graph(n, T, 1.0, 10.0, 0.1, seed=2).num_edges) / (n * T)
    assert d1 > d10
    with pytest.raises(ValueError, match="zeta R"):
        gnnmp.rand_temporal_hyperbolic_graph(10, 3, 1.0, 50.0, 0.1)
    with pytest.raises(TypeError, match="graph_type"):
        gnnmp.rand_temporal_radius_graph(10, 3, 0.1, 0.5, graph_type="sparse")


@gpu
@pytest.mark.parametrize("which", ["radius", "hyperbolic"])
def test_evolve_gcno_over_a_generated_temporal_graph(which):
    """5 snapshots x 30 nodes: the layer over the generated temporal graph (its kept batch) against the same layer over the same snapshots
    built one by one with GNNGraph(s, t) — tests/test_evolve_gcno.py's forward bound"""
    import gnnmp
    import torch
    T, N, cin, out = 5, 30, 4, 6
    if which == "radius":
        tg = gnnmp.rand_temporal_radius_graph(N, T, 0.1, 0.3, seed=5)
    else:
        tg = gnnmp.rand_temporal_hyperbolic_graph(N, T, 1.0, 4.0, 0.1, seed=5)
    assert tg._batched is not None and min(tg.num_edges) > 0
    by_hand = gnnmp.TemporalSnapshotsGNNGraph([gnnmp.GNNGraph(g.s.clone(), g.t.clone(), num_nodes=N) for g in tg])
    layer = gnnmp.EvolveGCNO((cin, out), seed=3)
    gen = torch.Generator(device="cuda").manual_seed(7)
    xs = [torch.randn((N, cin), generator=gen, device="cuda") for _ in range(T)]
    with torch.no_grad():
        ys, refs = layer(tg, xs), layer(by_hand, xs)
    for t, (y, ref) in enumerate(zip(ys, refs)):
        y, ref = y.cpu().numpy().astype(np.float64), ref.cpu().numpy().astype(np.float64)
        assert y.shape == (N, out) and np.all(np.isfinite(y))
        assert np.linalg.norm(y - ref) <= 1e-5 * np.linalg.norm(ref), t
        assert np.abs(y - ref).max() <= 1e-5 * np.abs(ref).max(), t
