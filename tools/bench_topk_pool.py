"""TopKPool timing: the pooled child graph (its plain plan) and the gated features, forward and forward + backward, the fused path against
the composition a user would write without it, in one process, alternating.
    <shape>.fwd.pool          gnnmp.topk_pool(l, g, x): gnnmp_topk_score_f32, gnnmp_topk_select_f32, gnnmp_plan_keep_nodes, gnnmp_topk_gate_f32
    <shape>.fwd.composed      the score in torch (x @ p / norm), a per-graph top-k by two stable torch.sort calls on (graph, -score),
                              gnnmp.remove_nodes with the dropped list, torch indexing and sigmoid for the gate
    <shape>.fwdbwd.pool       gnnmp.topk_pool_ad and the backward of a sum (gnnmp_topk_gate_grad_f32)
    <shape>.fwdbwd.composed   the composition under torch autograd
    <shape>.select.b<bytes>   gnnmp_topk_select_f32 alone at lds_budget_bytes = 1 KB (the default), 4 KB, 16 KB and 64 KB: the figures
                              behind the default budget (a member graph above the budget takes the device-memory route)
ratio = 0.5, C = 64.  Shapes: `qm9`, synth.batched_graphs(G = 4096, nmin = 9, nmax = 29); `clouds`, 32 clouds x 1024 points, knn_graph
k = 20; `arxiv`, the synth.arxiv_like hub graph, one graph (it takes the device-memory route at every budget).  Every path that builds a
child graph synchronises the host once, so this is WALL time between two device synchronisations, after --warmup calls, median of
--reps; rounds alternate the entries and every round is reported (a single run is a record, not a claim).  Before timing, the two paths
are compared: the same kept nodes, the same child edges, x2 within 1e-5.  Prints ONE JSON line.
    python tools/bench_topk_pool.py [--reps 20] [--warmup 3] [--rounds 2] [--arxiv-nodes 169343]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graphneuralnetworks.jl_amd"))

import gnnmp  # noqa: E402
from gnnmp import pool_topk, synth  # noqa: E402
from gnnmp.transform import _node_ptr  # noqa: E402

RATIO, C = 0.5, 64
BUDGETS = (1024, 4096, 16384, 65536)


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


def composed(g, x, p):
    """-> (g2, x2) as a user composes it today; differentiable in x and p through torch"""
    base, N = g.index_base, g.num_nodes
    y = x @ p / p.norm()
    yd = y.detach()
    if g.graph_indicator is not None and g.num_graphs > 1:
        gi0 = g.graph_indicator - base
        ptr = _node_ptr(g)
    else:
        gi0 = torch.zeros(N, dtype=torch.int64, device=x.device)
        ptr = torch.tensor([0, N], device=x.device)
    order = torch.sort(-yd, stable=True).indices
    order = order[torch.sort(gi0[order], stable=True).indices]               # by graph, then by descending score, ties by node id
    gs = gi0[order]
    rank = torch.arange(N, device=x.device) - ptr[gs]
    kg = torch.ceil(RATIO * (ptr[1:] - ptr[:-1]).double()).long()
    dropped = order[rank >= kg[gs]]
    g2 = gnnmp.remove_nodes(g, dropped + base)
    nid0 = g2.nid - base
    g2.plan(False)
    return g2, x[nid0] * torch.sigmoid(y[nid0])[:, None]


def fused(l, g, x):
    g2, x2 = gnnmp.topk_pool(l, g, x)
    g2.plan(False)
    return g2, x2


def fwdbwd_fused(l, g, x):
    xt = x.detach().requires_grad_(True)
    l.p = l.p.detach().requires_grad_(True)
    g2, x2 = gnnmp.topk_pool_ad(l, g, xt)
    x2.sum().backward()
    return xt.grad, l.p.grad


def fwdbwd_composed(l, g, x):
    xt = x.detach().requires_grad_(True)
    p = l.p.detach().requires_grad_(True)
    g2, x2 = composed(g, xt, p)
    x2.sum().backward()
    return xt.grad, p.grad


def check(l, g, x):
    ga, xa = fused(l, g, x)
    gb, xb = composed(g, x, l.p.detach())
    assert ga.num_nodes == gb.num_nodes
    if not torch.equal(ga.nid, gb.nid):      # the two scores round differently: a near-tie at rank k_g may fall either way
        assert int((ga.nid != gb.nid).sum()) <= 4, "the two paths keep different nodes"
        return
    assert torch.equal(ga.s, gb.s) and torch.equal(ga.t, gb.t)
    assert float((xa - xb).abs().max()) <= 1e-5 * float(xb.abs().max())


def shape_entries(tag, g, gen):
    x = torch.randn((g.num_nodes, C), generator=gen).cuda()
    l = gnnmp.TopKPool(RATIO, C, seed=1)
    g.plan(False)
    check(l, g, x)
    y = pool_topk.topk_score(x, l.p)
    entries = [(f"{tag}.fwd.pool", lambda: fused(l, g, x)), (f"{tag}.fwd.composed", lambda: composed(g, x, l.p.detach())),
               (f"{tag}.fwdbwd.pool", lambda: fwdbwd_fused(l, g, x)), (f"{tag}.fwdbwd.composed", lambda: fwdbwd_composed(l, g, x))]
    for b in BUDGETS:
        entries.append((f"{tag}.select.b{b}", lambda b=b: pool_topk.topk_select(y, 0, RATIO, g, "first", lds_budget_bytes=b)))
    return entries


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--arxiv-nodes", type=int, default=synth.ARXIV["N"])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_topk_pool needs a GPU: nothing is measured without one")
    gen = torch.Generator(device="cpu").manual_seed(1)
    qm9 = gnnmp.batch_arrays(synth.batched_graphs(G=4096, nmin=9, nmax=29, deg=2, seed=3))
    clouds_n, points, k = 32, 1024, 20
    pos = torch.rand((clouds_n * points, 3), generator=gen).cuda()
    gi = torch.arange(clouds_n).repeat_interleave(points).cuda() + 1
    clouds = gnnmp.knn_graph(pos, k, graph_indicator=gi)
    n = args.arxiv_nodes
    s, t = synth.arxiv_like(N=n, E=int(synth.ARXIV["E"] * n / synth.ARXIV["N"]), seed=7)
    arxiv = gnnmp.GNNGraph(torch.from_numpy(s).cuda(), torch.from_numpy(t).cuda(), num_nodes=n)
    shapes = (("qm9", qm9), ("clouds", clouds), ("arxiv", arxiv))
    entries = [e for tag, g in shapes for e in shape_entries(tag, g, gen)]
    rounds = []
    for _ in range(args.rounds):
        rounds.append({name: timed(fn, args.reps, args.warmup) for name, fn in entries})
    ms = {k_: min(r[k_] for r in rounds) for k_ in rounds[0]}
    ratios = {k_[:-len(".pool")] + ".composed_over_pool": ms[k_[:-len(".pool")] + ".composed"] / ms[k_] for k_ in ms if k_.endswith(".pool")}
    print(json.dumps({"tool": "bench_topk_pool", "device": torch.cuda.get_device_name(0), "reps": args.reps, "rounds": args.rounds,
                      "ratio": RATIO, "C": C,
                      "shapes": {tag: {"N": g.num_nodes, "E": g.num_edges, "graphs": g.num_graphs} for tag, g in shapes},
                      "ms_per_round": rounds, "ms": ms, "ratios": ratios}))


if __name__ == "__main__":
    main()
