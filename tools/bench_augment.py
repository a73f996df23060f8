"""Structural augmentation timing: the child graph WITH its three plans (plain, self-looped, transposed — what a GCNConv / GraphConv
training step on the augmented batch asks for), the derived path against the composition a user had before, in one process, alternating.
    <shape>.<aug>.derived    gnnmp.remove_nodes(g, p) / gnnmp.perturb_edges(g, ratio), then child.plan(False | True) and
                             child.plan_transposed(): gnnmp_plan_remove_nodes / gnnmp_plan_add_edges once per plan the parent has cached
    <shape>.<aug>.composed   the child's COO by torch indexing on the device (mask, cumsum, boolean indexing / randint, cat), then
                             gnnmp_plan_create three times (a sort and host synchronisations each)
Augmentations: remove_nodes at p = 0.1 and 0.5, perturb_edges at ratio 0.1 and 1.0.  Shapes: `qm9`, synth.batched_graphs(G = 4096,
nmin = 9, nmax = 29); `clouds`, 32 clouds x 1024 points, knn_graph k = 20; `arxiv`, the synth.arxiv_like hub graph of
tools/bench_poly_conv.py, bidirected.  Both paths synchronise the host, so this is WALL time between two device synchronisations, after
--warmup calls, median of --reps; rounds alternate the entries and every round is reported (a single run is a record, not a claim).
Before timing, the derived child's three plans are compared with plans built from its own COO (equal index arrays).  Prints ONE JSON line.
    python tools/bench_augment.py [--reps 20] [--warmup 3] [--rounds 2] [--arxiv-nodes 169343]"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graphneuralnetworks.jl_amd"))

import gnnmp  # noqa: E402
from gnnmp import synth  # noqa: E402
from gnnmp.graph import Plan  # noqa: E402


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def three_plans(s, t, n, base):
    return (Plan(s, t, n, n, base, False, validate=False), Plan(s, t, n, n, base, True, validate=False),
            Plan(t, s, n, n, base, False, validate=False))


def child_plans(c):
    return c.plan(False), c.plan(True), c.plan_transposed(False)


def composed_remove(g, p):
    n, base = g.num_nodes, g.index_base
    keep = torch.rand(n, device=g.device) >= p
    new = torch.cumsum(keep, 0) - 1 + base
    ek = keep[g.s - base] & keep[g.t - base]
    return three_plans(new[g.s[ek] - base], new[g.t[ek] - base], int(keep.sum()), base)


def composed_perturb(g, ratio):
    n, base, m = g.num_nodes, g.index_base, math.ceil(g.num_edges * ratio)
    sn = torch.randint(0, n, (m,), device=g.device)
    tn = torch.randint(0, n - 1, (m,), device=g.device)
    tn = tn + (tn >= sn)
    return three_plans(torch.cat([g.s, sn + base]), torch.cat([g.t, tn + base]), n, base)


def check(child):
    built = three_plans(child.s, child.t, child.num_nodes, child.index_base)
    for a, b in zip(child_plans(child), built):
        assert getattr(a, "_pooled", False), "the child's plan was not derived"
        for u, v in zip(a.export(), b.export()):
            assert torch.equal(u, v), "a derived plan differs from the plan built from the child's COO"


def shape_entries(tag, g):
    child_plans(g)                              # the parent's plans are cached, as in a training loop that convolves the clean batch too
    entries = []
    for p in (0.1, 0.5):
        check(gnnmp.remove_nodes(g, p, seed=5))
        entries.append((f"{tag}.remove_nodes_{p}.derived", lambda p=p: child_plans(gnnmp.remove_nodes(g, p))))
        entries.append((f"{tag}.remove_nodes_{p}.composed", lambda p=p: composed_remove(g, p)))
    for r in (0.1, 1.0):
        check(gnnmp.perturb_edges(g, r, seed=5))
        entries.append((f"{tag}.perturb_edges_{r}.derived", lambda r=r: child_plans(gnnmp.perturb_edges(g, r))))
        entries.append((f"{tag}.perturb_edges_{r}.composed", lambda r=r: composed_perturb(g, r)))
    return entries


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--arxiv-nodes", type=int, default=synth.ARXIV["N"])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_augment needs a GPU: nothing is measured without one")
    gen = torch.Generator(device="cpu").manual_seed(1)
    qm9 = gnnmp.batch_arrays(synth.batched_graphs(G=4096, nmin=9, nmax=29, deg=2, seed=3))
    clouds_n, points, k = 32, 1024, 20
    pos = torch.rand((clouds_n * points, 3), generator=gen).cuda()
    gi = torch.arange(clouds_n).repeat_interleave(points).cuda() + 1
    clouds = gnnmp.knn_graph(pos, k, graph_indicator=gi)
    n = args.arxiv_nodes
    s, t = synth.arxiv_like(N=n, E=int(synth.ARXIV["E"] * n / synth.ARXIV["N"]), seed=7)
    ring = np.arange(1, n + 1, dtype=np.int64)
    s, t = np.concatenate([s, ring]), np.concatenate([t, ring % n + 1])
    arxiv = gnnmp.to_bidirected(gnnmp.GNNGraph(torch.from_numpy(s).cuda(), torch.from_numpy(t).cuda(), num_nodes=n))
    shapes = (("qm9", qm9), ("clouds", clouds), ("arxiv", arxiv))
    entries = [e for tag, g in shapes for e in shape_entries(tag, g)]
    rounds = []
    for _ in range(args.rounds):
        rounds.append({name: timed(fn, args.reps, args.warmup) for name, fn in entries})
    ms = {k_: min(r[k_] for r in rounds) for k_ in rounds[0]}
    ratios = {k_[:-len(".derived")] + ".composed_over_derived": ms[k_[:-len(".derived")] + ".composed"] / ms[k_]
              for k_ in ms if k_.endswith(".derived")}
    print(json.dumps({"tool": "bench_augment", "device": torch.cuda.get_device_name(0), "reps": args.reps, "rounds": args.rounds,
                      "shapes": {tag: {"N": g.num_nodes, "E": g.num_edges, "max_in_degree": int(g.plan(False).max_degree)}
                                 for tag, g in shapes},
                      "ms_per_round": rounds, "ms": ms, "ratios": ratios}))


if __name__ == "__main__":
    main()
