"""EGNNConv timing at an n-body / molecule-like shape: the fused forward (gnnmp.egnn_conv_ad under torch.no_grad(): two dense calls on
N rows, gnnmp_egnn_edge_f32, the rest of ϕe and ϕx on E rows, one scatter, gnnmp_egnn_coord_f32, ϕh) against the existing composition
(gnnmp.egnn_conv: two [E][nin] gathers, a (2 nin + 1)-wide contraction on E rows, three [E][Dx] arrays, two scatters), and the trained
layer (gnnmp.egnn_conv_ad forward + backward: gradients of h, x and every weight and bias) — on the same device, in one process,
alternating A, B, C, A, B, C.
    fused_forward   gnnmp.egnn_conv_ad(l, g, h, x) under torch.no_grad()
    forward         gnnmp.egnn_conv(l, g, h, x) under torch.no_grad()                       the yardstick
    train           torch.autograd.backward(gnnmp.egnn_conv_ad(l, g, h, x), (Δh', Δx'))
Workload: 32 clouds x 1024 points in R^3, knn_graph k = 20 per cloud (E = 655 360, every destination row holds exactly 20 edges; the
largest OUT-degree is reported: the coordinate adjoint walks a source's row with one lane group), nin = hid = out = 64, residual, swish.
Device events after --warmup calls, median of --reps, rounds alternate the three; every round is reported (a single run is a record, not a
claim).  Before timing, the two forwards are compared at the timed size (norm-wise).  Prints ONE JSON line.
    python tools/bench_egnn_conv.py [--reps 20] [--warmup 3] [--rounds 2] [--clouds 32] [--points 1024] [--k 20]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graphneuralnetworks.jl_amd"))

import gnnmp  # noqa: E402

NIN = 64


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
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--clouds", type=int, default=32)
    ap.add_argument("--points", type=int, default=1024)
    ap.add_argument("--k", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_egnn_conv needs a GPU: nothing is measured without one")
    gen = torch.Generator(device="cpu").manual_seed(1)
    N = args.clouds * args.points
    pos = torch.rand((N, 3), generator=gen).cuda()
    gi = torch.arange(args.clouds).repeat_interleave(args.points).cuda() + 1
    g = gnnmp.knn_graph(pos, args.k, graph_indicator=gi)
    E = g.num_edges
    g.plan(False)
    pt = g.plan_transposed(False)
    h = (torch.rand((N, NIN), generator=gen) - 0.5).cuda()
    dh = (torch.rand((N, NIN), generator=gen) - 0.5).cuda()
    dx = (torch.rand((N, 3), generator=gen) - 0.5).cuda()
    l = gnnmp.EGNNConv((NIN, NIN), hidden_size=NIN, residual=True, seed=7)
    ps = [p for name in ("phi_e", "phi_x", "phi_h") for W, b, _ in getattr(l, name) for p in (W, b) if p is not None]
    hg, xg = h.clone().requires_grad_(True), pos.clone().requires_grad_(True)
    leaves = [hg, xg] + ps

    def fused_forward():
        with torch.no_grad():
            return gnnmp.egnn_conv_ad(l, g, h, pos)

    def forward():
        with torch.no_grad():
            return gnnmp.egnn_conv(l, g, h, pos)

    def train():
        for v in leaves:
            v.grad = None
        out = gnnmp.egnn_conv_ad(l, g, hg, xg)
        torch.autograd.backward(out, (dh, dx))
        return out

    rel = lambda a, b: float((a.double() - b.double()).norm() / b.double().norm())      # noqa: E731
    ref = forward()
    worst = max(rel(a, b) for a, b in zip(fused_forward(), ref))
    assert worst <= 1e-4, f"egnn_conv_ad's forward differs from gnnmp.egnn_conv by {worst:.2e} norm-wise"
    for p in ps:
        p.requires_grad_(True)
    worst = max([worst] + [rel(a.detach(), b) for a, b in zip(train(), ref)])
    assert all(v.grad is not None and bool(torch.isfinite(v.grad).all()) for v in leaves)
    rounds = []
    for _ in range(args.rounds):
        rounds.append({name: timed(fn, args.reps, args.warmup) for name, fn in (("fused_forward", fused_forward), ("forward", forward), ("train", train))})
    ms = {k: min(r[k] for r in rounds) for k in rounds[0]}
    print(json.dumps({"tool": "bench_egnn_conv", "device": torch.cuda.get_device_name(0), "reps": args.reps, "rounds": args.rounds, "N": N,
                      "E": E, "k": args.k, "Dx": 3, "nin": NIN, "hid": NIN, "max_out_degree": int(pt.max_degree),
                      "split_rows_transposed": int(pt.n_long), "residual": True, "ms_per_round": rounds, "ms": ms,
                      "forward_over_fused_forward": ms["forward"] / ms["fused_forward"], "worst_rel_between_forwards": worst}))


if __name__ == "__main__":
    main()
