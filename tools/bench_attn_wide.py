"""GATConv, GATv2Conv and TransformerConv at heads * out > 256 — rows wider than a wave, on the head-tiled kernels of csrc/attn_wide.hip —
against the same layer written in torch ops under torch autograd, on the same device, in one process, alternating.
    <layer>_forward        gnnmp.gatv2_conv / transformer_conv under torch.no_grad(); GAT: the forward of gat_conv_ad (it is the wide route)
    <layer>_forward_torch  dense calls, gathers to [E][H*C], the per-edge logit, scatter_reduce(amax) / index_add softmax and sum, no_grad
    gat_forward_3pass      gnnmp.gat_conv's inference forward: the three-pass kernels of csrc/attention.hip, the one wide route before
    <layer>_train          forward + backward of gat_conv_ad / gatv2_conv_ad / transformer_conv_ad: gradients of x and every weight
    <layer>_train_torch    the torch composition with torch autograd: what training these widths took before
Workloads, 64 channels in, add_self_loops = false, concat: `clouds` — 32 clouds x 1024 points in R^3, knn_graph k = 20 per cloud (every
destination row holds 20 edges); `arxiv` — synth.arxiv_like, a hub graph (the largest in- and out-degree are reported: a hub row is
walked by ONE wave a head tile).  Shapes 8 x 64 and 4 x 256.  Device events after --warmup calls, median of --reps, rounds alternate the
entries; every round is reported.  Before timing, outputs and gradients are compared at the timed size (norm-wise).  ONE JSON line.
    python tools/bench_attn_wide.py [--reps 10] [--warmup 2] [--rounds 2] [--clouds 32] [--points 1024] [--k 20] [--arxiv-nodes 169343]"""
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
from gnnmp.backward import gat_conv_ad  # noqa: E402
from gnnmp.backward_attn import gatv2_conv_ad, transformer_conv_ad  # noqa: E402
from gnnmp.layers_attn import GATv2Conv, TransformerConv, gatv2_conv, transformer_conv  # noqa: E402

NIN = 64
lin = torch.nn.functional.linear


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


def bench(g, H, C, args, gen):
    N, E = g.num_nodes, g.num_edges
    s0, t0 = (g.s - g.index_base).long(), (g.t - g.index_base).long()
    rnd = lambda *shape: (torch.rand(shape, generator=gen) - 0.5).cuda()      # noqa: E731
    x, dy = rnd(N, NIN), rnd(N, H * C)
    xg = x.clone().requires_grad_(True)
    gat = gnnmp.GATConv((NIN, C), "relu", heads=H, add_self_loops=False, seed=6)
    v2 = GATv2Conv((NIN, C), "relu", heads=H, add_self_loops=False, seed=7)
    tr = TransformerConv((NIN, C), heads=H, seed=8)

    def softmax_sum(logit, val):
        """α = softmax over each destination's in-edges of logit [E][H]; Σ_j α val [E][H][C] -> [N][H*C]"""
        mx = torch.full((N, H), -float("inf"), device=logit.device).scatter_reduce(0, t0[:, None].expand(E, H), logit, "amax")
        ex = torch.exp(logit - mx.detach()[t0])
        al = ex / torch.zeros((N, H), device=logit.device).index_add(0, t0, ex)[t0]
        return torch.zeros((N, H * C), device=logit.device).index_add(0, t0, (al.unsqueeze(-1) * val).reshape(E, H * C))

    def gat_torch(xv):
        Wx = lin(xv, gat.dense_x_weight).view(N, H, C)
        a = gat.a.t()                                                           # [H][2C]
        z = (Wx * a[None, :, :C]).sum(-1)[t0] + (Wx * a[None, :, C:]).sum(-1)[s0]
        return torch.relu(softmax_sum(torch.nn.functional.leaky_relu(z, gat.negative_slope), Wx[s0]) + gat.bias[None])

    def v2_torch(xv):
        Q, K = lin(xv, v2.dense_i_weight, v2.dense_i_bias).view(N, H, C), lin(xv, v2.dense_j_weight).view(N, H, C)
        Kj = K[s0]
        logit = (v2.a.t()[None] * torch.nn.functional.leaky_relu(Q[t0] + Kj, v2.negative_slope)).sum(-1)
        return torch.relu(softmax_sum(logit, Kj) + v2.bias[None])

    def tr_torch(xv):
        V, Q, K = (lin(xv, getattr(tr, f"W{k}_weight"), getattr(tr, f"W{k}_bias")).view(N, H, C) for k in "234")
        return softmax_sum((Q[t0] * K[s0]).sum(-1) / tr.sqrt_out, V[s0]) + lin(xv, tr.W1_weight, tr.W1_bias)

    def no_grad(fn):
        def run():
            with torch.no_grad():
                return fn()
        return run

    def train(fn, ps):
        def run():
            for v in [xg] + ps:
                v.grad = None
            out = fn()
            torch.autograd.backward(out, dy)
            return out
        return run

    layers = {"gat": (gat, lambda xv: gat_conv_ad(gat, g, xv), gat_torch), "gatv2": (v2, lambda xv: gatv2_conv_ad(v2, g, xv), v2_torch),
              "transformer": (tr, lambda xv: transformer_conv_ad(tr, g, xv), tr_torch)}
    fwd_fn = {"gat": lambda: gat_conv_ad(gat, g, x), "gatv2": lambda: gatv2_conv(v2, g, x), "transformer": lambda: transformer_conv(tr, g, x)}
    rel = lambda a, b: float((a.double() - b.double()).norm() / b.double().norm())      # noqa: E731
    entries, worst, worst_grad = {}, 0.0, 0.0
    for name, (l, ad, comp) in layers.items():
        ps = [p for p in l.parameters() if p is not None] if hasattr(l, "parameters") else [l.dense_x_weight, l.a, l.bias]
        entries[name + "_forward"], entries[name + "_forward_torch"] = no_grad(fwd_fn[name]), no_grad(lambda comp=comp: comp(x))
        worst = max(worst, rel(entries[name + "_forward"](), entries[name + "_forward_torch"]()))
        for p in ps:
            p.requires_grad_(True)
        entries[name + "_train"], entries[name + "_train_torch"] = train(lambda ad=ad: ad(xg), ps), train(lambda comp=comp: comp(xg), ps)
        entries[name + "_train"]()
        mine = [v.grad.clone() for v in [xg] + ps]
        entries[name + "_train_torch"]()
        for a, v in zip(mine, [xg] + ps):
            if float(v.grad.double().norm()) > 1e-3:      # (the key bias of the transformer has an identically vanishing gradient)
                worst_grad = max(worst_grad, rel(a, v.grad))
    entries["gat_forward_3pass"] = no_grad(lambda: gnnmp.gat_conv(gat, g, x))
    worst = max(worst, rel(entries["gat_forward"](), entries["gat_forward_3pass"]()))
    assert worst <= 1e-4, f"a forward differs from its torch composition by {worst:.2e} norm-wise"
    assert worst_grad <= 1e-3, f"a gradient differs from torch autograd on the composition by {worst_grad:.2e} norm-wise"
    rounds = [{name: timed(fn, args.reps, args.warmup) for name, fn in entries.items()} for _ in range(args.rounds)]
    ms = {k: min(r[k] for r in rounds) for k in rounds[0]}
    p, pt = g.plan(False), g.plan_transposed(False)
    return {"N": N, "E": E, "heads": H, "out": C, "max_in_degree": int(p.max_degree), "max_out_degree": int(pt.max_degree), "ms_per_round": rounds,
            "ms": ms, "torch_over_hip": {k: ms[k + "_torch"] / ms[k] for k in ms if k + "_torch" in ms},
            "three_pass_over_wide_gat_forward": ms["gat_forward_3pass"] / ms["gat_forward"], "worst_rel_between_forwards": worst,
            "worst_rel_between_gradients": worst_grad}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--clouds", type=int, default=32)
    ap.add_argument("--points", type=int, default=1024)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--arxiv-nodes", type=int, default=synth.ARXIV["N"])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_attn_wide needs a GPU: nothing is measured without one")
    gen = torch.Generator(device="cpu").manual_seed(1)
    N = args.clouds * args.points
    gi = torch.arange(args.clouds).repeat_interleave(args.points).cuda() + 1
    clouds = gnnmp.knn_graph(torch.rand((N, 3), generator=gen).cuda(), args.k, graph_indicator=gi)
    n = args.arxiv_nodes
    s, t = synth.arxiv_like(N=n, E=int(synth.ARXIV["E"] * n / synth.ARXIV["N"]), seed=7)
    arxiv = gnnmp.GNNGraph(torch.from_numpy(s).cuda(), torch.from_numpy(t).cuda(), num_nodes=n)
    res = {f"{gname}_{H}x{C}": bench(g, H, C, args, gen) for gname, g in (("clouds", clouds), ("arxiv", arxiv)) for H, C in ((8, 64), (4, 256))}
    print(json.dumps({"tool": "bench_attn_wide", "device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup,
                      "rounds": args.rounds, "nin": NIN, "results": res}))


if __name__ == "__main__":
    main()
