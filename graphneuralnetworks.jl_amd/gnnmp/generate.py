"""The temporal graph generators rand_temporal_radius_graph and rand_temporal_hyperbolic_graph (GNNGraphs/src/generate.jl:265-380) and
their deterministic building block hyperbolic_graph.

The reference builds one snapshot after the other on the CPU: a tree search (radius) or an N x N Float64 loop into a dense adjacency
(hyperbolic) per snapshot.  Here the T snapshots are ONE batch — the [T N, 2] positions with the snapshot as graph_indicator — searched
ONCE on the device (gnnmp_radius_graph_f32 / gnnmp_hyperbolic_graph_f32, include/gnnmp.h states the predicate and its error bound); the
snapshots are cut from the batch's plan with gnnmp_plan_select (no sort, no host synchronisation per snapshot: the T edge counts are
read in one copy), and the searched batch is kept as the temporal graph's batched() form, which is what EvolveGCNO aggregates over.

The trajectories are T N numbers: torch ops on the caller's device, in float64, rounded to float32 once.  Each generator is a pure
function of explicit uniform draws (radius_trajectory / hyperbolic_trajectory, which run on CPU tensors too) behind a thin wrapper that
draws them from a torch.Generator seeded with `seed`: the same seed gives a bit-identical temporal graph.  It is NOT Julia's RNG stream.
"""
from __future__ import annotations

import ctypes
import math

import torch

from . import _lib as L
from .graph import GNNGraph, Plan
from .neighbors import _graph, _indicator_args, _prepare, _status, radius_graph
from .temporal_graph import TemporalSnapshotsGNNGraph

# include/gnnmp.h, gnnmp_hyperbolic_graph_f32: every pair value is finite in float32 while zeta r <= 44 for all nodes (r <= R here)
MAX_ZETA_R = 44.0


def hyperbolic_graph(points, R, zeta=1.0, graph_indicator=None, self_loops=False, index_base=1, idx_dtype=torch.int64, **kws) -> GNNGraph:
    """Every node of the hyperbolic plane is linked to the points (of its own graph) within hyperbolic distance R at curvature parameter
    zeta — the adjacency loop of rand_temporal_hyperbolic_graph (generate.jl:287-297, 359-369) as one device search.  points: (num_nodes,
    2) float32 rows (r, theta); theta is any real angle.  The graph is symmetric; edges are ordered as GNNGraph(adj) orders them (targets
    ascend, sources ascend within a target) and carry float32 weights 1, as the reference's dense adjacency does.  kws go to GNNGraph."""
    R, zeta = float(R), float(zeta)
    if not R >= 0.0:
        raise ValueError(f"hyperbolic_graph: R = {R} (negative or NaN)")
    if not (zeta > 0.0 and math.isfinite(zeta)):
        raise ValueError(f"hyperbolic_graph: zeta = {zeta} (not finite, or <= 0)")
    x, n, gi, G, device = _prepare(points, graph_indicator, "in", index_base, idx_dtype)
    if x.shape[1] != 2:
        raise ValueError("hyperbolic_graph: points are (r, theta) rows")
    h = ctypes.c_void_p()
    _status(L.load().gnnmp_hyperbolic_graph_f32(ctypes.byref(h), L.ptr(x), n, ctypes.c_float(R), ctypes.c_float(zeta),
                                                *_indicator_args(gi, index_base, G), int(bool(self_loops)), L.stream_ptr()))
    g = _graph(h, n, gi, G, "in", index_base, idx_dtype, device, kws)
    if g.w is None:
        g.w = torch.ones(g.num_edges, dtype=torch.float32, device=device)       # GNNGraph(adj) keeps A[nz] (convert.jl:75-95)
    return g


# ---- trajectories: pure functions of the uniform draws ----------------------------------------------------------------------------------
def radius_trajectory(u0, u_rho, u_theta, speed, dtype=torch.float32):
    """positions [T, N, 2] float32 of rand_temporal_radius_graph (generate.jl:272-281, as the code has it) from uniform draws in [0, 1):
    u0 [N, 2] the first positions, u_rho / u_theta [T - 1, N] the steps: rho = 2 speed u - speed, theta = 2 pi u,
    x <- 1 - |1 - |x + rho cos theta||, y likewise with sin.  Snapshot t holds the positions before the t-th update.  float64 inside,
    rounded to `dtype` once at the end."""
    pos = u0.to(torch.float64)
    rho = 2.0 * float(speed) * u_rho.to(torch.float64) - float(speed)
    th = 2.0 * math.pi * u_theta.to(torch.float64)
    step = torch.stack((rho * torch.cos(th), rho * torch.sin(th)), dim=-1)      # [T - 1, N, 2]
    out = [pos]
    for k in range(step.shape[0]):
        pos = 1.0 - torch.abs(1.0 - torch.abs(pos + step[k]))
        out.append(pos)
    return torch.stack(out).to(dtype)


def hyperbolic_trajectory(u_p, u_theta0, u_dp, u_dtheta, alpha, R, speed, return_p=False, dtype=torch.float32):
    """positions [T, N, 2] float32, rows (r, theta), of rand_temporal_hyperbolic_graph (generate.jl:351-377) from uniform draws in
    [0, 1): u_p / u_theta0 [N] the first quantiles and angles (theta = 2 pi u), u_dp / u_dtheta [T - 1, N] the steps (2 speed u - speed).
    r = acosh(1 + (cosh(alpha R) - 1) p) / alpha;  p <- p + step, then p > 1 -> 1 - (p mod 1) and p < 0 -> |p|;  theta <- theta + step,
    never wrapped.  float64 inside, rounded to `dtype` once at the end.  return_p: also the quantiles [T, N] in float64."""
    alpha, R, speed = float(alpha), float(R), float(speed)
    p = u_p.to(torch.float64)
    th = 2.0 * math.pi * u_theta0.to(torch.float64)
    dp = 2.0 * speed * u_dp.to(torch.float64) - speed
    dth = 2.0 * speed * u_dtheta.to(torch.float64) - speed
    scale = math.cosh(alpha * R) - 1.0
    ps, out = [], []
    for k in range(dp.shape[0] + 1):
        ps.append(p)
        out.append(torch.stack((torch.acosh(1.0 + scale * p) / alpha, th), dim=-1))
        if k < dp.shape[0]:
            p = p + dp[k]
            p = torch.where(p > 1.0, 1.0 - torch.fmod(p, 1.0), p)
            p = torch.where(p < 0.0, torch.abs(p), p)
            th = th + dth[k]
    pts = torch.stack(out).to(dtype)
    return (pts, torch.stack(ps)) if return_p else pts


def _draws(seed, device, *shapes):
    """float64 uniforms in [0, 1) from one torch.Generator on `device`, seeded with `seed` (None: a fresh random seed)"""
    gen = torch.Generator(device=device)
    if seed is None:
        gen.seed()
    else:
        gen.manual_seed(int(seed))
    return [torch.rand(s, generator=gen, dtype=torch.float64, device=device) for s in shapes]


# ---- one search, T cuts --------------------------------------------------------------------------------------------------------------------
def _graph_kws(who, kws):
    index_base, idx_dtype = kws.pop("index_base", 1), kws.pop("idx_dtype", torch.int64)
    if kws:
        raise TypeError(f"{who}: unsupported keyword {sorted(kws)[0]!r} (index_base and idx_dtype are passed on)")
    return index_base, idx_dtype


def _snapshot_indicator(T, N, index_base, idx_dtype, device):
    return torch.arange(index_base, T + index_base, dtype=idx_dtype, device=device).repeat_interleave(N)


def _cut_snapshots(gb, T, N, dir, weighted):
    """the T snapshots of the searched batch `gb` (snapshot t = its rows t N .. (t + 1) N) and the temporal graph that keeps gb"""
    dev, base = gb.device, gb.index_base
    key = False if dir == "in" else ("T", False)
    plan = gb._plans[key]
    lib = L.load()
    # the snapshots' edge counts: the batch's row pointer at the T + 1 boundaries, ONE copy to the host
    rowptr = torch.empty(T * N + 1, dtype=torch.int64, device=dev)
    L.check(lib.gnnmp_plan_export64(plan.handle, L.ptr(rowptr), None, None, L.stream_ptr()))
    bounds = rowptr[::N].cpu().tolist()
    node_ptr = torch.arange(T + 1, dtype=torch.int64, device=dev) * N
    ids = torch.arange(base, T + base, dtype=torch.int64, device=dev)
    ones = gb.w if weighted else None                                            # (the batch's weights: ones)
    idx_dtype = gb.s.dtype
    snaps = []
    for t in range(T):
        e0, e1 = bounds[t], bounds[t + 1]
        h = ctypes.c_void_p()
        L.check(lib.gnnmp_plan_select(ctypes.byref(h), plan.handle, L.ptr(node_ptr), T, L.ptr(ids[t:t + 1]), 8, base, 1, N, e1 - e0,
                                      None, None, None, L.stream_ptr()))
        p = Plan._adopt(h, dev)
        g = GNNGraph._from_plan(p, 1, None, None, base, idx_dtype)
        if dir == "out":                 # the cut is the plan of the REVERSED edges: rows are the sources
            g._plans = {key: p}
            g._t, g._s = p.edge_index(idx_dtype, base)
        if weighted:
            g.w = ones[e0:e1]
        snaps.append(g)
    tg = TemporalSnapshotsGNNGraph(snaps)
    tg._batched = (snaps[0], [0, N]) if T == 1 else (gb, [t * N for t in range(T + 1)])
    return tg


def temporal_radius_graph(points, r, self_loops=False, dir="in", index_base=1, idx_dtype=torch.int64):
    """the temporal graph of given positions [T, N, 2]: snapshot t = radius_graph(points[t], r), all T found by one search"""
    T, N = int(points.shape[0]), int(points.shape[1])
    flat = points.reshape(T * N, 2)
    gb = radius_graph(flat, r, _snapshot_indicator(T, N, index_base, idx_dtype, flat.device), self_loops=self_loops, dir=dir,
                      index_base=index_base, idx_dtype=idx_dtype)
    return _cut_snapshots(gb, T, N, dir, False)


def temporal_hyperbolic_graph(points, R, zeta=1.0, self_loops=False, index_base=1, idx_dtype=torch.int64):
    """the temporal graph of given positions [T, N, 2], rows (r, theta): snapshot t = hyperbolic_graph(points[t], R, zeta)"""
    T, N = int(points.shape[0]), int(points.shape[1])
    flat = points.reshape(T * N, 2)
    gb = hyperbolic_graph(flat, R, zeta, _snapshot_indicator(T, N, index_base, idx_dtype, flat.device), self_loops=self_loops,
                          index_base=index_base, idx_dtype=idx_dtype)
    return _cut_snapshots(gb, T, N, "in", True)


def _sizes(who, number_nodes, number_snapshots):
    N, T = int(number_nodes), int(number_snapshots)
    if N < 1 or T < 1:
        raise ValueError(f"{who}: number_nodes = {N} and number_snapshots = {T} must be positive")
    return N, T


def rand_temporal_radius_graph(number_nodes, number_snapshots, speed, r, self_loops=False, dir="in", seed=None, return_points=False,
                               **kws):
    """rand_temporal_radius_graph(number_nodes, number_snapshots, speed, r; self_loops = false, dir = :in, kws...) — generate.jl:265-284:
    points uniform in the unit square, linked within distance r; every snapshot moves each point by a random vector of length up to
    `speed` and bounces it off the walls.  Returns a TemporalSnapshotsGNNGraph whose batched() form is already there; return_points:
    also the positions [T, N, 2] float32.  The same `seed` gives a bit-identical temporal graph (torch's generator on the device, not
    Julia's RNG stream).  kws: index_base, idx_dtype."""
    L.require_gpu()
    who = "rand_temporal_radius_graph"
    N, T = _sizes(who, number_nodes, number_snapshots)
    r = float(r)
    if not r >= 0.0:
        raise ValueError(f"{who}: r = {r} (negative or NaN)")
    assert dir in ("in", "out"), "dir must be :in or :out"
    index_base, idx_dtype = _graph_kws(who, dict(kws))
    dev = torch.device("cuda", torch.cuda.current_device())
    u0, u_rho, u_theta = _draws(seed, dev, (N, 2), (T - 1, N), (T - 1, N))
    pts = radius_trajectory(u0, u_rho, u_theta, speed)
    tg = temporal_radius_graph(pts, r, self_loops, dir, index_base, idx_dtype)
    return (tg, pts) if return_points else tg


def rand_temporal_hyperbolic_graph(number_nodes, number_snapshots, alpha, R, speed, zeta=1, self_loop=False, seed=None,
                                   return_points=False, **kws):
    """rand_temporal_hyperbolic_graph(number_nodes, number_snapshots; α, R, speed, ζ = 1, self_loop = false, kws...) — generate.jl:340-380:
    points quasi-uniform (parameter alpha) in the hyperbolic disk of radius R, linked within hyperbolic distance R; every snapshot moves
    the radial quantile and the angle of each point by up to `speed`.  Returns a TemporalSnapshotsGNNGraph (snapshots carry weights 1, as
    GNNGraph(adj) does) whose batched() form is already there; return_points: also the positions [T, N, 2] float32, rows (r, theta).
    The same `seed` gives a bit-identical temporal graph (torch's generator on the device, not Julia's RNG stream).
    kws: index_base, idx_dtype."""
    assert int(number_snapshots) > 1, "The number of snapshots must be greater than 1"
    assert alpha > 0, "α must be greater than 0"
    L.require_gpu()
    who = "rand_temporal_hyperbolic_graph"
    N, T = _sizes(who, number_nodes, number_snapshots)
    R, zeta = float(R), float(zeta)
    if not R >= 0.0:
        raise ValueError(f"{who}: R = {R} (negative or NaN)")
    if not (zeta > 0.0 and math.isfinite(zeta)):
        raise ValueError(f"{who}: zeta = {zeta} (not finite, or <= 0)")
    if zeta * R > MAX_ZETA_R:
        raise ValueError(f"{who}: zeta R = {zeta * R} > {MAX_ZETA_R}: pair values overflow float32")
    index_base, idx_dtype = _graph_kws(who, dict(kws))
    dev = torch.device("cuda", torch.cuda.current_device())
    u_p, u_th, u_dp, u_dth = _draws(seed, dev, (N,), (N,), (T - 1, N), (T - 1, N))
    pts = hyperbolic_trajectory(u_p, u_th, u_dp, u_dth, alpha, R, speed)
    tg = temporal_hyperbolic_graph(pts, R, zeta, self_loop, index_base, idx_dtype)
    return (tg, pts) if return_points else tg
