"""MEGNetConv timing at a point-cloud shape: the existing composition (gnnmp.megnet_conv: two [E][in] gathers, a 2 in-wide contraction
on E rows, a dense on e, an add and a bias_act before the first hidden layer exists) against the fused forward (gnnmp.megnet_conv_ad under
torch.no_grad(): two dense calls on N rows, one on E rows, gnnmp_megnet_edge_f32) and the trained layer (forward + backward: gradients
of x, e and every weight and bias of ϕe and ϕv) — and the two new row steps alone, each against the composition it replaces — on the same
device, in one process, alternating.
    forward          gnnmp.megnet_conv(l, g, x, e) under torch.no_grad()                         the yardstick
    fused_forward    gnnmp.megnet_conv_ad(l, g, x, e) under torch.no_grad()
    train            torch.autograd.backward(gnnmp.megnet_conv_ad(l, g, x, e), (Δx̄, Δē))
    edge_grad_fused  gnnmp_megnet_edge_grad_f32: dz0, dP, dQ from Δa0 and a0 (relu)                one call, two passes
    edge_grad_comp   gnnmp_act_grad_z_f32, then gnnmp_scatter_f32 over the plan and over the transposed plan
    aggr_grad_fused  gnnmp_aggregate_grad_f32 (mean) with acc = Δē                                one pass
    aggr_grad_comp   gnnmp_mul_rows_f32 by 1 / deg on N rows, gnnmp_gather_f32 to E rows, gnnmp_add_f32 with Δē
Workload: 32 clouds x 1024 points in R^3, knn_graph k = 20 per cloud (E = 655 360, every destination row holds exactly 20 edges; the
largest OUT-degree is reported: pass 2 of the edge-head pullback walks a source's row with one lane group), 64 channels, e = 64 edge
features, MEGNetConv(64 => 64), mean.  Device events after --warmup calls, median of --reps, rounds alternate the entries; every round is
reported (a single run is a record, not a claim).  Before timing, the forwards and the row steps are compared at the timed size
(norm-wise).  Prints ONE JSON line.
    python tools/bench_megnet_conv.py [--reps 20] [--warmup 3] [--rounds 2] [--clouds 32] [--points 1024] [--k 20]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graphneuralnetworks.jl_amd"))

import gnnmp  # noqa: E402
from gnnmp import _lib as L  # noqa: E402
from gnnmp.backward_egnn import act_grad_z  # noqa: E402
from gnnmp.backward_megnet import aggregate_grad, megnet_edge_grad  # noqa: E402
from gnnmp.layers_more import _add  # noqa: E402
from gnnmp.msgpass import _gather, _scatter_plan  # noqa: E402

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
        raise SystemExit("bench_megnet_conv needs a GPU: nothing is measured without one")
    gen = torch.Generator(device="cpu").manual_seed(1)
    N = args.clouds * args.points
    pos = torch.rand((N, 3), generator=gen).cuda()
    gi = torch.arange(args.clouds).repeat_interleave(args.points).cuda() + 1
    g = gnnmp.knn_graph(pos, args.k, graph_indicator=gi)
    E = g.num_edges
    plan, pt = g.plan(False), g.plan_transposed(False)
    rnd = lambda *shape: (torch.rand(shape, generator=gen) - 0.5).cuda()      # noqa: E731
    x, e, dxb, deb = rnd(N, NIN), rnd(E, NIN), rnd(N, NIN), rnd(E, NIN)
    l = gnnmp.MEGNetConv((NIN, NIN), aggr="mean", seed=7)
    ps = [p for d in list(l.phi_e) + list(l.phi_v) for p in (d.weight, d.bias) if p is not None]
    xg, eg = x.clone().requires_grad_(True), e.clone().requires_grad_(True)
    leaves = [xg, eg] + ps

    def forward():
        with torch.no_grad():
            return gnnmp.megnet_conv(l, g, x, e)

    def fused_forward():
        with torch.no_grad():
            return gnnmp.megnet_conv_ad(l, g, x, e)

    def train():
        for v in leaves:
            v.grad = None
        out = gnnmp.megnet_conv_ad(l, g, xg, eg)
        torch.autograd.backward(out, (dxb, deb))
        return out

    # the row steps alone: Δa0 and a0 = relu(z0) of the edge head; Δxᵉ [N] and Δē [E] of the edge output
    da0, a0 = rnd(E, NIN), torch.relu(rnd(E, NIN)).contiguous()
    inv_deg = (1.0 / torch.bincount(g.t - g.index_base, minlength=N).clamp(min=1).float()).contiguous()

    def edge_grad_fused():
        return megnet_edge_grad(plan, pt, da0, a0, L.ACT_RELU, True, True)

    def edge_grad_comp():
        dz0 = act_grad_z(da0, a0, L.ACT_RELU)
        return dz0, _scatter_plan("+", dz0, plan), _scatter_plan("+", dz0, pt)

    def aggr_grad_fused():
        return aggregate_grad(plan, "mean", dxb, acc=deb)

    def aggr_grad_comp():
        scaled = torch.empty_like(dxb)
        L.check(L.load().gnnmp_mul_rows_f32(L.ptr(inv_deg), 1, L.ptr(dxb), L.ptr(scaled), N, NIN, L.stream_ptr()))
        return _add(deb, _gather(scaled, g.t, g.index_base))

    rel = lambda a, b: float((a.double() - b.double()).norm() / b.double().norm())      # noqa: E731
    ref = forward()
    worst = max(rel(a, b) for a, b in zip(fused_forward(), ref))
    assert worst <= 1e-4, f"megnet_conv_ad's forward differs from gnnmp.megnet_conv by {worst:.2e} norm-wise"
    for p in ps:
        p.requires_grad_(True)
    worst = max([worst] + [rel(a.detach(), b) for a, b in zip(train(), ref)])
    assert all(v.grad is not None and bool(torch.isfinite(v.grad).all()) for v in leaves)
    worst_rows = max([rel(a, b) for a, b in zip(edge_grad_fused(), edge_grad_comp())] + [rel(aggr_grad_fused(), aggr_grad_comp())])
    assert worst_rows <= 1e-5, f"a fused row step differs from its composition by {worst_rows:.2e} norm-wise"
    entries = (("forward", forward), ("fused_forward", fused_forward), ("train", train), ("edge_grad_fused", edge_grad_fused),
               ("edge_grad_comp", edge_grad_comp), ("aggr_grad_fused", aggr_grad_fused), ("aggr_grad_comp", aggr_grad_comp))
    rounds = []
    for _ in range(args.rounds):
        rounds.append({name: timed(fn, args.reps, args.warmup) for name, fn in entries})
    ms = {k: min(r[k] for r in rounds) for k in rounds[0]}
    print(json.dumps({"tool": "bench_megnet_conv", "device": torch.cuda.get_device_name(0), "reps": args.reps, "rounds": args.rounds, "N": N,
                      "E": E, "k": args.k, "nin": NIN, "out": NIN, "aggr": "mean", "max_out_degree": int(pt.max_degree),
                      "split_rows_transposed": int(pt.n_long), "ms_per_round": rounds, "ms": ms,
                      "forward_over_fused_forward": ms["forward"] / ms["fused_forward"],
                      "edge_grad_comp_over_fused": ms["edge_grad_comp"] / ms["edge_grad_fused"],
                      "aggr_grad_comp_over_fused": ms["aggr_grad_comp"] / ms["aggr_grad_fused"],
                      "worst_rel_between_forwards": worst, "worst_rel_between_row_steps": worst_rows}))


if __name__ == "__main__":
    main()
