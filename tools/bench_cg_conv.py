"""CGConv timing at a CGCNN-like shape: the fused forward (gnnmp.cg_conv), the trained layer (gnnmp.cg_conv_ad forward + backward: three
dense calls, gnnmp_propagate_cg_f32, the two passes of csrc/cg_grad.hip, the dense adjoints on N and E rows) and a torch-autograd
composition of the reference's body on E rows — on the same device, in one process, alternating A, B, C, A, B, C.  Per (nin, out):
    forward      gnnmp.cg_conv(l, g, x, e) under torch.no_grad()
    train        gnnmp.cg_conv_ad(l, g, x, e).backward(Δ)                    gradients of x, e, both weights, both biases
    torch_train  index_select, cat, two matmul, sigmoid * softplus, index_add_, + x; .backward(Δ)       the same gradients by autograd
Workload: 32 clouds x 1024 points in R^3, knn_graph k = 12 per cloud (E = 393 216, every destination row holds exactly 12 edges; the
largest OUT-degree is reported: sources are the only possible hubs, and the gradient passes walk a hub row with one lane group),
x [N][nin] and e [E][16] uniform, act = softplus, residual.
Device events after --warmup calls, median of --reps, rounds alternate the three; every round is reported (a single run is a record, not a
claim).  Before timing, the layer's y and gradients are compared with torch's at the timed size (norm-wise).  Prints ONE JSON line.
    python tools/bench_cg_conv.py [--reps 20] [--warmup 3] [--rounds 2] [--clouds 32] [--points 1024] [--k 12]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graphneuralnetworks.jl_amd"))

import gnnmp  # noqa: E402

SHAPES = ((64, 64), (128, 128))
EIN = 16


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
    ap.add_argument("--k", type=int, default=12)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_cg_conv needs a GPU: nothing is measured without one")
    gen = torch.Generator(device="cpu").manual_seed(1)
    N = args.clouds * args.points
    pos = torch.rand((N, 3), generator=gen).cuda()
    gi = torch.arange(args.clouds).repeat_interleave(args.points).cuda() + 1
    g = gnnmp.knn_graph(pos, args.k, graph_indicator=gi)
    E = g.num_edges
    g.plan(False)
    pt = g.plan_transposed(False)
    s0, t0 = g.s - 1, g.t - 1
    out = {"tool": "bench_cg_conv", "device": torch.cuda.get_device_name(0), "reps": args.reps, "rounds": args.rounds, "N": N, "E": E,
           "k": args.k, "ein": EIN, "max_out_degree": int(pt.max_degree), "split_rows_transposed": int(pt.n_long), "act": "softplus",
           "residual": True, "shapes": {}}
    for nin, C in SHAPES:
        x = (torch.rand((N, nin), generator=gen) - 0.5).cuda()
        e = (torch.rand((E, EIN), generator=gen) - 0.5).cuda()
        dy = (torch.rand((N, C), generator=gen) - 0.5).cuda()
        l = gnnmp.CGConv(((nin, EIN), C), "softplus", residual=True, seed=nin + C)
        l.dense_f_bias.uniform_(-0.1, 0.1)
        l.dense_s_bias.uniform_(-0.1, 0.1)
        ps = [l.dense_f_weight, l.dense_s_weight, l.dense_f_bias, l.dense_s_bias]
        for p in ps:
            p.requires_grad_(True)
        xg, eg = x.clone().requires_grad_(True), e.clone().requires_grad_(True)
        leaves = [xg, eg] + ps

        def forward():
            with torch.no_grad():
                return gnnmp.cg_conv(l, g, x, e)

        def train():
            for v in leaves:
                v.grad = None
            y = gnnmp.cg_conv_ad(l, g, xg, eg)
            y.backward(dy)
            return y

        def torch_train():
            for v in leaves:
                v.grad = None
            z = torch.cat([xg.index_select(0, t0), xg.index_select(0, s0), eg], dim=1)
            m = torch.sigmoid(z @ l.dense_f_weight.t() + l.dense_f_bias) * torch.nn.functional.softplus(z @ l.dense_s_weight.t() + l.dense_s_bias)
            y = torch.zeros((N, C), device="cuda").index_add_(0, t0, m) + xg
            y.backward(dy)
            return y

        rel = lambda a, b: float((a.double() - b.double()).norm() / b.double().norm())      # noqa: E731
        y_t = torch_train().detach()
        g_t = [v.grad.clone() for v in leaves]
        y_f = train().detach()
        worst = max([rel(y_f, y_t), rel(forward(), y_t)] + [rel(v.grad, r) for v, r in zip(leaves, g_t)])
        assert worst <= 1e-4, f"(nin, out) = ({nin}, {C}): cg_conv_ad differs from torch's float32 autograd by {worst:.2e} norm-wise"
        rounds = []
        for _ in range(args.rounds):
            rounds.append({name: timed(fn, args.reps, args.warmup) for name, fn in (("forward", forward), ("train", train), ("torch_train", torch_train))})
        out["shapes"][f"nin{nin}_out{C}"] = {"ms_per_round": rounds, "ms": {k: min(r[k] for r in rounds) for k in rounds[0]},
                                            "worst_rel_vs_torch_fp32": worst}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
