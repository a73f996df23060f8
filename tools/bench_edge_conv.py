"""EdgeConv timing at a DGCNN shape: the fused pair-message path (gnnmp.edge_conv_ad: one dense call on N rows + one pass of
edge_conv_rows_kernel, csrc/edge_conv.hip) against the unchanged composition it stands beside (gnnmp.edge_conv: gather, edge_sub, the
dense on E rows, scatter) — on the same device, in one process, A, B, A, B.  Per (D, C):
    composition   gnnmp.edge_conv(l, g, x)                                  the reference's literal statement order on E-row arrays
    fused         gnnmp.edge_conv_ad(l, g, x) under torch.no_grad()         the fused forward
    fused_train   edge_conv_ad forward + backward (Δ given)                 dense, rows kernel, the two gradient passes, dense adjoints
Workload: 32 clouds x 1024 points in R^3, knn_graph k = 20 per cloud (E = 655 360, every destination row holds exactly 20 edges; the
largest OUT-degree is reported: sources are the only possible hubs), features [N][D] uniform, nn = Dense(2D => C, relu), aggr = max.
Device events after warm-up, median of --reps, the better of two rounds.  Algorithmic bytes (4-byte words, every array counted once per
pass that reads or writes it, indices included):
    composition   7 E D + 2 E C + N C + 3 E            gather (r + w), edge_sub (2 r + w), dense on E rows (2 r, w E C), scatter (r E C + idx, w N C)
    fused         N D + 4 N C + E C + E + N C          dense (r N D, w 2 N C), rows kernel (r 2 N C own rows + E C gathered + E idx, w N C)
    fused_train   fused + the dst pass (E C + E + 4 N C + N C) + the src pass (4 E C + E + N C + 2 N C) + the dense adjoints (2 (2 N C) + 2 N D)
Before timing, the fused forward is compared with the composition at the timed size (norm-wise).  Prints ONE JSON line.
    python tools/bench_edge_conv.py [--reps 20] [--warmup 3] [--clouds 32] [--points 1024] [--k 20]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graphneuralnetworks.jl_amd"))

import gnnmp  # noqa: E402

SHAPES = ((3, 64), (64, 64), (64, 128), (128, 256))


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
    ap.add_argument("--clouds", type=int, default=32)
    ap.add_argument("--points", type=int, default=1024)
    ap.add_argument("--k", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_edge_conv needs a GPU: nothing is measured without one")
    gen = torch.Generator(device="cpu").manual_seed(1)
    N = args.clouds * args.points
    pos = torch.rand((N, 3), generator=gen).cuda()
    gi = torch.arange(args.clouds).repeat_interleave(args.points).cuda() + 1
    g = gnnmp.knn_graph(pos, args.k, graph_indicator=gi)
    E = g.num_edges
    g.plan(False)
    pt = g.plan_transposed(False)
    out = {"tool": "bench_edge_conv", "device": torch.cuda.get_device_name(0), "reps": args.reps, "N": N, "E": E, "k": args.k,
           "max_out_degree": int(pt.max_degree), "split_rows_transposed": int(pt.n_long), "aggr": "max", "sigma": "relu", "shapes": {}}
    for D, C in SHAPES:
        x = pos if D == 3 else torch.rand((N, D), generator=gen).cuda()
        dy = torch.rand((N, C), generator=gen).cuda()
        l = gnnmp.EdgeConv(gnnmp.Dense((2 * D, C), "relu", seed=D + C), aggr="max")
        l.nn.weight.requires_grad_(True)
        l.nn.bias.requires_grad_(True)
        xg = x.clone().requires_grad_(True)

        def composition():
            with torch.no_grad():
                return gnnmp.edge_conv(l, g, x)

        def fused():
            with torch.no_grad():
                return gnnmp.edge_conv_ad(l, g, x)

        def fused_train():
            xg.grad = l.nn.weight.grad = l.nn.bias.grad = None
            gnnmp.edge_conv_ad(l, g, xg).backward(dy)

        yc, yf = composition().double(), fused().double()
        rel = float((yc - yf).norm() / yc.norm())
        assert rel <= 1e-5, f"(D, C) = ({D}, {C}): the fused forward differs from the composition by {rel:.2e} norm-wise"
        ms = {}
        for rnd in range(2):
            for name, fn in (("fused", fused), ("composition", composition), ("fused_train", fused_train)):
                t = timed(fn, args.reps, args.warmup)
                ms[name] = t if rnd == 0 else min(ms[name], t)
        words = {"composition": 7 * E * D + 2 * E * C + N * C + 3 * E,
                 "fused": N * D + 4 * N * C + E * C + E + N * C}
        words["fused_train"] = words["fused"] + (E * C + E + 5 * N * C) + (4 * E * C + E + 3 * N * C) + (4 * N * C + 2 * N * D)
        out["shapes"][f"D{D}_C{C}"] = {"ms": ms, "algorithmic_MB": {k: 4 * v / 1e6 for k, v in words.items()},
                                      "algorithmic_GBps": {k: 4 * words[k] / ms[k] / 1e6 for k in ms},
                                      "forward_speedup": ms["composition"] / ms["fused"], "fused_vs_composition_rel": rel}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
