"""GATv2Conv and TransformerConv WITH edge features at a point-cloud shape: the fused layers (csrc/attn_edge.hip) against the composition
a user could write before them, on the same device, in one process, alternating.
    gatv2_forward / transformer_forward      gnnmp.gatv2_conv(l, g, x, e) / gnnmp.transformer_conv(l, g, x, e) under torch.no_grad()
    gatv2_forward_comp / transformer_..._comp the dense calls, then gathers to [E][H*C] arrays, the per-edge message in torch, gnnmp's
                                             softmax_edge_neighbors and aggregate_neighbors (apply_edges' generic path), no_grad
    gatv2_train / transformer_train          forward + backward of gatv2_conv_ad / transformer_conv_ad: gradients of x, e and every weight
    gatv2_train_comp / transformer_train_comp the same composition in differentiable torch (index_select, scatter_reduce(amax), index_add)
                                             with torch autograd: what training these layers with e took before
Workload: 32 clouds x 1024 points in R^3, knn_graph k = 20 per cloud (E = 655 360, every destination row holds 20 edges; the largest
OUT-degree is reported: pass 2 of the pullback walks a source's row with one lane group), 64 channels in, heads = 4 of 16 channels,
ein = 16, concat.  Device events after --warmup calls, median of --reps, rounds alternate the entries; every round is reported (a single
run is a record, not a claim).  Before timing, fused and composed results are compared at the timed size (norm-wise).  ONE JSON line.
    python tools/bench_attn_edge.py [--reps 20] [--warmup 3] [--rounds 2] [--clouds 32] [--points 1024] [--k 20]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graphneuralnetworks.jl_amd"))

import gnnmp  # noqa: E402
from gnnmp.backward_attn import gatv2_conv_ad, transformer_conv_ad  # noqa: E402
from gnnmp.layers import dense  # noqa: E402
from gnnmp.layers_attn import GATv2Conv, TransformerConv, gatv2_conv, transformer_conv  # noqa: E402

NIN, H, C, EIN = 64, 4, 16, 16


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
        raise SystemExit("bench_attn_edge needs a GPU: nothing is measured without one")
    gen = torch.Generator(device="cpu").manual_seed(1)
    N = args.clouds * args.points
    pos = torch.rand((N, 3), generator=gen).cuda()
    gi = torch.arange(args.clouds).repeat_interleave(args.points).cuda() + 1
    g = gnnmp.knn_graph(pos, args.k, graph_indicator=gi)
    E = g.num_edges
    s0, t0 = (g.s - g.index_base).long(), (g.t - g.index_base).long()
    rnd = lambda *shape: (torch.rand(shape, generator=gen) - 0.5).cuda()      # noqa: E731
    x, e, dy = rnd(N, NIN), rnd(E, EIN), rnd(N, H * C)
    gat = GATv2Conv(((NIN, EIN), C), "relu", heads=H, add_self_loops=False, seed=7)
    tr = TransformerConv(((NIN, EIN), C), heads=H, seed=8)
    xg, eg = x.clone().requires_grad_(True), e.clone().requires_grad_(True)

    def lin(v, W, b=None, grad=False):
        """the dense call of the layer: gnnmp's kernel without autograd, torch's with"""
        return torch.nn.functional.linear(v, W, b) if grad else dense(v, W, b)

    def softmax_sum(logit, val, grad):
        """α = softmax over each destination's in-edges of logit [E][H]; Σ_j α val [E][H][C] -> [N][H*C]"""
        if not grad:
            al = gnnmp.softmax_edge_neighbors(g, logit.contiguous())
            return gnnmp.aggregate_neighbors(g, "+", (al.unsqueeze(-1) * val).reshape(E, H * C).contiguous())
        mx = torch.full((N, H), -float("inf"), device=logit.device).scatter_reduce(0, t0[:, None].expand(E, H), logit, "amax")
        ex = torch.exp(logit - mx.detach()[t0])
        den = torch.zeros((N, H), device=logit.device).index_add(0, t0, ex)
        al = ex / den[t0]
        return torch.zeros((N, H * C), device=logit.device).index_add(0, t0, (al.unsqueeze(-1) * val).reshape(E, H * C))

    def gat_comp(xv, ev, grad):
        Q, K, F = lin(xv, gat.dense_i_weight, gat.dense_i_bias, grad), lin(xv, gat.dense_j_weight, None, grad), lin(ev, gat.dense_e_weight, None, grad)
        Kj = K[s0].view(E, H, C)
        z = Q[t0].view(E, H, C) + Kj + F.view(E, H, C)
        logit = (gat.a.t()[None] * torch.nn.functional.leaky_relu(z, gat.negative_slope)).sum(-1)
        return torch.relu(softmax_sum(logit, Kj, grad) + gat.bias[None])

    def tr_comp(xv, ev, grad):
        V, Q, K = (lin(xv, getattr(tr, f"W{k}_weight"), getattr(tr, f"W{k}_bias"), grad) for k in "234")
        F = lin(ev, tr.W6_weight, tr.W6_bias, grad).view(E, H, C)
        logit = (Q[t0].view(E, H, C) * (K[s0].view(E, H, C) + F)).sum(-1) / tr.sqrt_out
        return softmax_sum(logit, V[s0].view(E, H, C) + F, grad) + lin(xv, tr.W1_weight, tr.W1_bias, grad)

    gat_ps, tr_ps = [p for p in gat.parameters() if p is not None], [p for p in tr.parameters() if p is not None]

    def no_grad(fn):
        def run():
            with torch.no_grad():
                return fn()
        return run

    def train(fn, ps):
        def run():
            for v in [xg, eg] + ps:
                v.grad = None
            out = fn()
            torch.autograd.backward(out, dy)
            return out
        return run

    rel = lambda a, b: float((a.double() - b.double()).norm() / b.double().norm())      # noqa: E731
    fwd = {"gatv2_forward": no_grad(lambda: gatv2_conv(gat, g, x, e)), "gatv2_forward_comp": no_grad(lambda: gat_comp(x, e, False)),
           "transformer_forward": no_grad(lambda: transformer_conv(tr, g, x, e)),
           "transformer_forward_comp": no_grad(lambda: tr_comp(x, e, False))}
    worst = max(rel(fwd["gatv2_forward"](), fwd["gatv2_forward_comp"]()), rel(fwd["transformer_forward"](), fwd["transformer_forward_comp"]()))
    assert worst <= 1e-4, f"a fused forward differs from its composition by {worst:.2e} norm-wise"
    for p in gat_ps + tr_ps:
        p.requires_grad_(True)
    trn = {"gatv2_train": train(lambda: gatv2_conv_ad(gat, g, xg, eg), gat_ps), "gatv2_train_comp": train(lambda: gat_comp(xg, eg, True), gat_ps),
           "transformer_train": train(lambda: transformer_conv_ad(tr, g, xg, eg), tr_ps),
           "transformer_train_comp": train(lambda: tr_comp(xg, eg, True), tr_ps)}
    worst_grad = 0.0
    for name, ps in (("gatv2_train", gat_ps), ("transformer_train", tr_ps)):
        trn[name]()
        fused = [v.grad.clone() for v in [xg, eg] + ps]
        trn[name + "_comp"]()
        for a, v in zip(fused, [xg, eg] + ps):
            if float(v.grad.double().norm()) > 1e-3:      # (the key bias of the transformer has an identically vanishing gradient)
                worst_grad = max(worst_grad, rel(a, v.grad))
    assert worst_grad <= 1e-3, f"a fused gradient differs from torch autograd on the composition by {worst_grad:.2e} norm-wise"
    entries = list(fwd.items()) + list(trn.items())
    rounds = []
    for _ in range(args.rounds):
        rounds.append({name: timed(fn, args.reps, args.warmup) for name, fn in entries})
    ms = {k: min(r[k] for r in rounds) for k in rounds[0]}
    pt = g.plan_transposed(False)
    print(json.dumps({"tool": "bench_attn_edge", "device": torch.cuda.get_device_name(0), "reps": args.reps, "rounds": args.rounds, "N": N,
                      "E": E, "k": args.k, "nin": NIN, "heads": H, "out": C, "ein": EIN, "max_out_degree": int(pt.max_degree),
                      "split_rows_transposed": int(pt.n_long), "ms_per_round": rounds, "ms": ms,
                      "comp_over_fused": {k: ms[k + "_comp"] / ms[k] for k in ("gatv2_forward", "gatv2_train", "transformer_forward",
                                                                               "transformer_train")},
                      "worst_rel_between_forwards": worst, "worst_rel_between_gradients": worst_grad}))


if __name__ == "__main__":
    main()
