"""TGCN timing: the one-launch recurrence (csrc/temporal.hip) against the per-step path (knob 20 < 0), forward and forward + backward,
on three shapes — (a) the traffic-prediction example's (207 sensors, ~1.7k edges, TGCN(2 => 100), T = 3), (b) a batch of 64 such graphs at
T = 12, (c) one road-like graph of ~70k nodes at T = 12, out = 100.  Device-event timing after warm-up (median of --reps); prints ONE JSON
line with per shape fused / per-step ms and the largest relative difference between the two paths' outputs.
    python tools/bench_tgcn.py [--reps 20] [--warmup 5] [--shapes a,b,c]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graphneuralnetworks.jl_amd"))

import gnnmp  # noqa: E402
from gnnmp import _lib  # noqa: E402


def road(n, deg=8, seed=0):
    """ring + chords to the next few nodes, bidirected, 1-based (the shape of a sensor network's k-nearest graph)"""
    rng = np.random.default_rng(seed)
    i = np.repeat(np.arange(n), deg // 2)
    j = (i + rng.integers(1, 12, i.size)) % n
    e = np.unique(np.stack([np.concatenate([i, j]), np.concatenate([j, i])], 1), axis=0)
    return e[:, 0].astype(np.int64) + 1, e[:, 1].astype(np.int64) + 1


def graph(kind):
    if kind == "a":
        s, t = road(207, seed=1)
        return gnnmp.GNNGraph(torch.from_numpy(s).cuda(), torch.from_numpy(t).cuda(), num_nodes=207), 3
    if kind == "b":
        gs = []
        for k in range(64):
            s, t = road(207, seed=10 + k)
            gs.append(gnnmp.GNNGraph(torch.from_numpy(s).cuda(), torch.from_numpy(t).cuda(), num_nodes=207))
        return gnnmp.batch(gs), 12
    s, t = road(70000, seed=2)
    return gnnmp.GNNGraph(torch.from_numpy(s).cuda(), torch.from_numpy(t).cuda(), num_nodes=70000), 12


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--shapes", default="a,b,c")
    a = ap.parse_args()
    res = {"bench": "tgcn", "device": torch.cuda.get_device_name(0), "shapes": {}}
    for kind in a.shapes.split(","):
        g, T = graph(kind)
        layer = gnnmp.TGCN((2, 100), seed=1)
        for p in layer.cell.parameters():
            p.requires_grad_()
        x = torch.randn((g.num_nodes, T, 2), device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))
        dy = torch.ones((g.num_nodes, T, 100), device="cuda")
        params = layer.cell.parameters()

        def fwd():
            return layer(g, x)

        def fwdbwd():
            xd = x.detach().requires_grad_()
            y = gnnmp.tgcn_ad(layer, g, xd)
            return torch.autograd.grad(y, [xd] + params, dy)

        row = {"N": g.num_nodes, "E": g.num_edges, "T": T, "in": 2, "out": 100}
        outs = {}
        for path, kv in (("fused", 0), ("per_step", -1)):
            _lib.tune(_lib.Knob.TGCN, kv)
            try:
                row[path + "_fwd_ms"] = timed(fwd, a.reps, a.warmup)
                row[path + "_fwdbwd_ms"] = timed(fwdbwd, a.reps, a.warmup)
                outs[path] = [fwd()] + list(fwdbwd())
            finally:
                _lib.tune(_lib.Knob.TGCN, 0)
        row["max_rel_diff"] = max(float((u - v).abs().max() / v.abs().max().clamp(min=1e-30))
                                  for u, v in zip(outs["fused"], outs["per_step"]))
        row["fwd_speedup"] = row["per_step_fwd_ms"] / row["fused_fwd_ms"]
        row["fwdbwd_speedup"] = row["per_step_fwdbwd_ms"] / row["fused_fwdbwd_ms"]
        res["shapes"][kind] = row
    print(json.dumps(res))


if __name__ == "__main__":
    main()
