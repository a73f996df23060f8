"""ChebConv, DConv and GatedGraphConv timing: the existing forwards (gnnmp.cheb_conv: six launches an order; gnnmp.d_conv: three a step and
direction) against the fused forwards (gnnmp.cheb_conv_ad / gnnmp.d_conv_ad under torch.no_grad(): ONE gnnmp_poly_hop_f32 launch an order)
and the trained layers (forward + backward: gradients of x and every weight and bias), plus the GRU pullback alone and the trained
GatedGraphConv — on the same device, in one process, alternating.
    cheb_forward        gnnmp.cheb_conv(l, g, x) under torch.no_grad(), k = 3                       the yardstick
    cheb_fused_forward  gnnmp.cheb_conv_ad(l, g, x) under torch.no_grad()
    cheb_train          gnnmp.cheb_conv_ad(l, g, x).backward(Δ)
    dconv_forward       gnnmp.d_conv(l, g, x) under torch.no_grad(), k = 2                          the yardstick
    dconv_fused_forward gnnmp.d_conv_ad(l, g, x) under torch.no_grad()
    dconv_train         gnnmp.d_conv_ad(l, g, x).backward(Δ)
    gru_grad            gnnmp_gru_pointwise_grad_f32 alone on [N][64]
    ggc_forward         gnnmp.gated_graph_conv(l, g, x), 2 layers, +
    ggc_train           gnnmp.gated_graph_conv_ad(l, g, x).backward(Δ)
Workloads, 64 channels: `clouds` — 32 clouds x 1024 points in R^3, knn_graph k = 20 per cloud, made bidirected; `arxiv` — one
synth.arxiv_like graph (a ring added so that no node is isolated), made bidirected: its hubs are rows that the existing forwards split
and the fused hop walks with one lane group, so the price of whole-row walks is on record beside the gain.  Device events after --warmup
calls, median of --reps, rounds alternate the entries; every round is reported (a single run is a record, not a claim).  Before timing,
the forwards are compared at the timed size (norm-wise).  Prints ONE JSON line.
    python tools/bench_poly_conv.py [--reps 20] [--warmup 3] [--rounds 2] [--clouds 32] [--points 1024] [--k 20] [--arxiv-nodes 169343]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graphneuralnetworks.jl_amd"))

import gnnmp  # noqa: E402
from gnnmp import synth  # noqa: E402
from gnnmp.backward_gated import gru_pointwise_grad  # noqa: E402

C = 64


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


def workload(name, g, args, gen):
    N = g.num_nodes
    rnd = lambda *shape: (torch.rand(shape, generator=gen) - 0.5).cuda()      # noqa: E731
    x, dy = rnd(N, C), rnd(N, C)
    cheb, dconv, ggc = gnnmp.ChebConv((C, C), 3, seed=3), gnnmp.DConv((C, C), 2, seed=5), gnnmp.GatedGraphConv(C, 2, seed=9)
    params = [cheb.weight, cheb.bias, dconv.weights, dconv.bias, ggc.weight, ggc.gru_Wi, ggc.gru_Wh, ggc.gru_b]
    xg = x.clone().requires_grad_(True)

    def plain(fn, l):
        def run():
            with torch.no_grad():
                return fn(l, g, x)
        return run

    def train(fn, l):
        def run():
            for v in [xg] + params:
                v.grad = None
            out = fn(l, g, xg)
            out.backward(dy)
            return out
        return run

    gx, gh, b, h = rnd(N, 3 * C), rnd(N, 3 * C), rnd(3 * C), rnd(N, C)
    rel = lambda a, b_: float((a.double() - b_.double()).norm() / b_.double().norm())      # noqa: E731
    worst = max(rel(plain(gnnmp.cheb_conv_ad, cheb)(), plain(gnnmp.cheb_conv, cheb)()),
                rel(plain(gnnmp.d_conv_ad, dconv)(), plain(gnnmp.d_conv, dconv)()))
    assert worst <= 1e-4, f"{name}: a fused forward differs from the existing one by {worst:.2e} norm-wise"
    assert torch.equal(plain(gnnmp.gated_graph_conv_ad, ggc)(), plain(gnnmp.gated_graph_conv, ggc)())
    for p in params:
        p.requires_grad_(True)
    entries = (("cheb_forward", plain(gnnmp.cheb_conv, cheb)), ("cheb_fused_forward", plain(gnnmp.cheb_conv_ad, cheb)),
               ("cheb_train", train(gnnmp.cheb_conv_ad, cheb)),
               ("dconv_forward", plain(gnnmp.d_conv, dconv)), ("dconv_fused_forward", plain(gnnmp.d_conv_ad, dconv)),
               ("dconv_train", train(gnnmp.d_conv_ad, dconv)),
               ("gru_grad", lambda: gru_pointwise_grad(gx, gh, b, h, dy)),
               ("ggc_forward", plain(gnnmp.gated_graph_conv, ggc)), ("ggc_train", train(gnnmp.gated_graph_conv_ad, ggc)))
    for _, fn in entries:      # every path once: caches on the graph (slot factors, λmax), and a check that the gradients exist
        fn()
    assert all(v.grad is not None and bool(torch.isfinite(v.grad).all()) for v in [xg] + params[4:])
    rounds = []
    for _ in range(args.rounds):
        rounds.append({k: timed(fn, args.reps, args.warmup) for k, fn in entries})
    ms = {k: min(r[k] for r in rounds) for k in rounds[0]}
    plan, pt = g.plan(False), g.plan_transposed(False)
    return {"N": N, "E": g.num_edges, "max_in_degree": int(plan.max_degree), "max_out_degree": int(pt.max_degree),
            "split_rows": int(plan.n_long), "split_rows_transposed": int(pt.n_long), "ms_per_round": rounds, "ms": ms,
            "cheb_forward_over_fused": ms["cheb_forward"] / ms["cheb_fused_forward"],
            "dconv_forward_over_fused": ms["dconv_forward"] / ms["dconv_fused_forward"],
            "worst_rel_between_forwards": worst}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--clouds", type=int, default=32)
    ap.add_argument("--points", type=int, default=1024)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--arxiv-nodes", type=int, default=synth.ARXIV["N"])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_poly_conv needs a GPU: nothing is measured without one")
    gen = torch.Generator(device="cpu").manual_seed(1)
    N = args.clouds * args.points
    pos = torch.rand((N, 3), generator=gen).cuda()
    gi = torch.arange(args.clouds).repeat_interleave(args.points).cuda() + 1
    clouds = gnnmp.to_bidirected(gnnmp.knn_graph(pos, args.k, graph_indicator=gi))
    n = args.arxiv_nodes
    s, t = synth.arxiv_like(N=n, E=int(synth.ARXIV["E"] * n / synth.ARXIV["N"]), seed=7)
    ring = np.arange(1, n + 1, dtype=np.int64)
    s, t = np.concatenate([s, ring]), np.concatenate([t, ring % n + 1])
    arxiv = gnnmp.to_bidirected(gnnmp.GNNGraph(torch.from_numpy(s).cuda(), torch.from_numpy(t).cuda(), num_nodes=n))
    out = {"tool": "bench_poly_conv", "device": torch.cuda.get_device_name(0), "reps": args.reps, "rounds": args.rounds, "channels": C,
           "cheb_k": 3, "dconv_k": 2, "ggc_layers": 2, "clouds": workload("clouds", clouds, args, gen),
           "arxiv": workload("arxiv", arxiv, args, gen)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
