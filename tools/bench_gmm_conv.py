"""GMMConv timing at a MoNet-like point-cloud shape: the composed forward (gnnmp.gmm_conv: gnnmp_gmm_weights_f32 broadcast to [E][K out],
dense, gnnmp_propagate_emul_f32 on [N][K out], gnnmp_head_mean_f32), the fused forward (gnnmp.gmm_conv_ad under no_grad:
gnnmp_gmm_weights_f32 with C = 1, dense, gnnmp_gmm_conv_f32 of csrc/gmm.hip) and the trained layer (gnnmp.gmm_conv_ad forward + backward)
— on the same device, in one process, alternating A, B, C, A, B, C:
    composed     gnnmp.gmm_conv(l, g, x, e) under torch.no_grad()
    fused        gnnmp.gmm_conv_ad(l, g, x, e) under torch.no_grad()
    train        gnnmp.gmm_conv_ad(l, g, x, e).backward(Δ)                gradients of x, e, mu, sigma_inv, dense_x_weight, bias
    rows_*       the row steps alone, on the same w / xk: gnnmp_propagate_emul_f32 + gnnmp_head_mean_f32 against gnnmp_gmm_conv_f32
Workload: 32 clouds x 1024 points in R^3, knn_graph k = 20 per cloud (E = 655 360, every destination row holds exactly 20 edges; the
largest OUT-degree is reported: sources are the only possible hubs, and the pullback walks a hub row with one lane group), e = the
relative positions (ein = 3), K = 3, in = out = 64, σ = relu, bias.
Device events after --warmup calls, median of --reps, rounds alternate the entries; every round is reported (a single run is a record, not
a claim).  Before timing, the fused y is compared with the composed y at the timed size (norm-wise).  Prints ONE JSON line.
    python tools/bench_gmm_conv.py [--reps 20] [--warmup 3] [--rounds 2] [--clouds 32] [--points 1024] [--k 20] [--K 3] [--dim 64]"""
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
from gnnmp import backward_gmm as BG  # noqa: E402


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
    ap.add_argument("--K", type=int, default=3)
    ap.add_argument("--dim", type=int, default=64)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_gmm_conv needs a GPU: nothing is measured without one")
    gen = torch.Generator(device="cpu").manual_seed(1)
    N, K, D = args.clouds * args.points, args.K, args.dim
    pos = torch.rand((N, 3), generator=gen).cuda()
    gi = torch.arange(args.clouds).repeat_interleave(args.points).cuda() + 1
    g = gnnmp.knn_graph(pos, args.k, graph_indicator=gi)
    E = g.num_edges
    plan = g.plan(False)
    pt = g.plan_transposed(False)
    e = (pos[g.s - 1] - pos[g.t - 1]).contiguous()
    x = (torch.rand((N, D), generator=gen) - 0.5).cuda()
    dy = (torch.rand((N, D), generator=gen) - 0.5).cuda()
    l = gnnmp.GMMConv(((D, 3), D), "relu", K=K, seed=7)
    l.bias.uniform_(-0.1, 0.1)
    ps = [l.mu, l.sigma_inv, l.dense_x_weight, l.bias]
    xg, eg = x.clone().requires_grad_(True), e.clone().requires_grad_(True)
    leaves = [xg, eg] + ps
    lib = L.load()

    def composed():
        with torch.no_grad():
            return gnnmp.gmm_conv(l, g, x, e)

    def fused():
        with torch.no_grad():
            return gnnmp.gmm_conv_ad(l, g, x, e)

    def train():
        for v in leaves:
            v.grad = None
        y = gnnmp.gmm_conv_ad(l, g, xg, eg)
        y.backward(dy)
        return y

    # the row steps alone, on fixed operands
    with torch.no_grad():
        xk = gnnmp.layers.dense(x, l.dense_x_weight)
        w1 = BG.gmm_weights(e, l.mu, l.sigma_inv)
        wb = torch.empty((E, K * D), dtype=torch.float32, device="cuda")
        L.check(lib.gnnmp_gmm_weights_f32(L.ptr(e), L.ptr(l.mu), L.ptr(l.sigma_inv), L.ptr(wb), E, 3, K, D, L.stream_ptr()))
    m = torch.empty((N, K * D), dtype=torch.float32, device="cuda")
    yr = torch.empty((N, D), dtype=torch.float32, device="cuda")

    def rows_composed():
        L.check(lib.gnnmp_propagate_emul_f32(plan.handle, L.MEAN, L.ptr(xk), L.ptr(wb), L.ptr(m), K * D, L.stream_ptr()))
        L.check(lib.gnnmp_head_mean_f32(L.ptr(m), L.ptr(l.bias), L.ACT_RELU, L.ptr(yr), N, K, D, L.stream_ptr()))

    def rows_fused():
        return BG.gmm_rows(plan, w1, xk, l.bias, L.ACT_RELU, K, D, False)[0]

    rel = lambda a, b: float((a.double() - b.double()).norm() / b.double().norm())      # noqa: E731
    y_c = composed()
    rows_composed()
    worst = max(rel(fused(), y_c), rel(rows_fused(), yr))
    assert worst <= 1e-5, f"the fused forward differs from gnnmp.gmm_conv by {worst:.2e} norm-wise"
    for p in ps:
        p.requires_grad_(True)
    assert rel(train().detach(), y_c) <= 1e-5 and all(v.grad is not None and bool(torch.isfinite(v.grad).all()) for v in leaves)
    entries = (("composed", composed), ("fused", fused), ("train", train), ("rows_composed", rows_composed), ("rows_fused", rows_fused))
    rounds = []
    for _ in range(args.rounds):
        rounds.append({name: timed(fn, args.reps, args.warmup) for name, fn in entries})
    out = {"tool": "bench_gmm_conv", "device": torch.cuda.get_device_name(0), "reps": args.reps, "rounds": args.rounds, "N": N, "E": E,
           "k": args.k, "ein": 3, "K": K, "in": D, "out": D, "act": "relu", "max_out_degree": int(pt.max_degree),
           "split_rows_transposed": int(pt.n_long), "ms_per_round": rounds, "ms": {k: min(r[k] for r in rounds) for k in rounds[0]},
           "worst_rel_fused_vs_composed": worst}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
