"""Temporal-graph construction timing, from GIVEN positions [T, N, 2] (the trajectories are T N numbers of torch arithmetic and are left out):
    (a) per_snapshot   T calls of gnnmp.radius_graph, one a snapshot, + TemporalSnapshotsGNNGraph + tg.batched() (gnnmp.batch): the only
                       way before the generators existed
    (b) batched        gnnmp.generate.temporal_radius_graph: ONE search over the [T N, 2] batch, T gnnmp_plan_select cuts, the searched
                       batch kept as tg.batched()
    (c) hyperbolic     gnnmp.hyperbolic_graph on the [T N, 2] batch against torch: the same predicate evaluated on a [T, N, N] float32
                       array (cosh(zeta dr) + 2 sinh sinh sin^2(dtheta / 2), dtheta formed in float64) + nonzero + GNNGraph's plan build
Both sides of (a) / (b) end with the T snapshot graphs, their plans and the batched graph; both sides of (c) with the batch's graph and
its plan.  A, B, A, B in one process, device events after warm-up, median of --reps; every entry synchronises inside (plan builds do),
so the times are whole-call times, not kernel times.  Prints ONE JSON line.
    python tools/bench_temporal_graphs.py [--reps 20] [--warmup 3] [--shapes small,mid,large]"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graphneuralnetworks.jl_amd"))

import gnnmp  # noqa: E402
from gnnmp import generate as G  # noqa: E402

#         name     T    N     r (mean degree ~ pi r^2 N)   hyperbolic R (alpha = zeta = 1)
SHAPES = (("small", 5, 30, 0.3, 4.0), ("mid", 16, 1024, 0.06, 10.0), ("large", 32, 4096, 0.03, 14.0))


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def torch_hyperbolic(pts, T, N, R, zeta):
    """the batch's graph through torch: the predicate on a [T, N, N] array, nonzero, GNNGraph + its plan build (a sort)"""
    r, th = pts[..., 0], pts[..., 1].double()
    sh = torch.sinh(zeta * r)
    half = torch.sin((th[:, :, None] - th[:, None, :]) * 0.5).float()
    v = torch.cosh(zeta * (r[:, :, None] - r[:, None, :])) + 2.0 * sh[:, :, None] * sh[:, None, :] * half * half
    v.diagonal(dim1=1, dim2=2).fill_(float("inf"))
    snap, centre, nb = torch.nonzero(v <= math.cosh(zeta * R), as_tuple=True)
    off = snap * N + 1
    g = gnnmp.GNNGraph(nb + off, centre + off, num_nodes=T * N, _validated=True)
    g.plan(False)
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default="small,mid,large")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_temporal_graphs needs the GPU: there is no CPU fallback and no CPU timing"
    out = {"bench": "temporal_graphs", "reps": a.reps, "shapes": {}}
    for name, T, N, r, R in SHAPES:
        if name not in a.shapes.split(","):
            continue
        u = G._draws(7, torch.device("cuda"), (N, 2), (T - 1, N), (T - 1, N), (N,), (N,), (T - 1, N), (T - 1, N))
        pts = G.radius_trajectory(u[0], u[1], u[2], 0.05)
        hpts = G.hyperbolic_trajectory(u[3], u[4], u[5], u[6], 1.0, R, 0.05)
        hflat = hpts.reshape(T * N, 2)
        gi = G._snapshot_indicator(T, N, 1, torch.int64, hflat.device)

        def per_snapshot():
            tg = gnnmp.TemporalSnapshotsGNNGraph([gnnmp.radius_graph(pts[t], r) for t in range(T)])
            return tg, tg.batched()

        def batched():
            tg = G.temporal_radius_graph(pts, r)
            return tg, tg.batched()

        def hyp_ours():
            return gnnmp.hyperbolic_graph(hflat, R, 1.0, gi)

        def hyp_torch():
            return torch_hyperbolic(hpts, T, N, R, 1.0)

        row = {"T": T, "N": N, "r": r, "R": R}
        for rnd in range(2):                                      # A, B, A, B: the spread between the rounds is the box noise
            for key, fn in (("per_snapshot_ms", per_snapshot), ("batched_ms", batched), ("hyperbolic_ms", hyp_ours),
                            ("torch_hyperbolic_ms", hyp_torch)):
                row.setdefault(key, []).append(timed(fn, a.reps, a.warmup))
        (tga, _), (tgb, _) = per_snapshot(), batched()
        row["edges"] = int(sum(tgb.num_edges))
        row["same_graphs"] = bool(tga == tgb)
        go, gt = hyp_ours(), hyp_torch()
        row["hyperbolic_edges"] = [int(go.num_edges), int(gt.num_edges)]     # (torch's float32 value has no error bound: the counts may differ)
        row["batched_speedup"] = min(row["per_snapshot_ms"]) / min(row["batched_ms"])
        row["hyperbolic_speedup"] = min(row["torch_hyperbolic_ms"]) / min(row["hyperbolic_ms"])
        out["shapes"][name] = row
    print(json.dumps(out))


if __name__ == "__main__":
    main()
