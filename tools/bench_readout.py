"""Attention readout timing at two shapes, 64 channels: the existing compositions (gnnmp.set2set_pool: per iteration broadcast_nodes,
rowdot, softmax_nodes, mul_rows, reduce_nodes; gnnmp.global_attention_pool: softmax_nodes, mul_rows, reduce_nodes) against the fused
forwards (gnnmp.set2set_ad / gnnmp.global_attention_pool_ad under torch.no_grad(): one gnnmp_segment_attn_pool_f32 per softmax-weighted
sum) and the trained readouts (forward + backward) against the same readout written in torch ops with torch autograd on the device — what
a user could do before — in one process, alternating.
    s2s_forward        gnnmp.set2set_pool(l, g, x) under torch.no_grad()                           the yardstick
    s2s_fused_forward  gnnmp.set2set_ad(l, g, x) under torch.no_grad()
    s2s_train          gnnmp.set2set_ad forward + backward: gradients of x, Wi, Wh, b
    s2s_torch_train    the same in torch ops (index_select, scatter_reduce, index_add) with torch autograd
    gap_forward        gnnmp.global_attention_pool(l, g, x) under torch.no_grad()                  the yardstick
    gap_fused_forward  gnnmp.global_attention_pool_ad(l, g, x) under torch.no_grad()
    gap_train          gnnmp.global_attention_pool_ad forward + backward: gradients of x and of fgate's and ffeat's weights and biases
    gap_torch_train    the same in torch ops with torch autograd
Shapes: `qm9`, synth.batched_graphs(G = 4096, nmin = 9, nmax = 29) — molecules of 9 to 29 atoms; `clouds`, 32 clouds x 1024 points (ONE
lane group walks each cloud: 32 lane groups on the whole device — the documented weak spot).  Set2Set with 3 iterations;
GlobalAttentionPool(fgate = Dense(64 => 1), ffeat = Dense(64 => 64, relu)).  Device events after --warmup calls, median of --reps, rounds
alternate the entries; every round is reported (a single run is a record, not a claim).  Before timing, the forwards and the gradients are
compared at the timed size (norm-wise).  Prints ONE JSON line.
    python tools/bench_readout.py [--reps 20] [--warmup 3] [--rounds 2]"""
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
from gnnmp.layers_khop import GlobalAttentionPool  # noqa: E402

D, ITERS = 64, 3


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


def segment_softmax(s, gi, G):
    """softmax_nodes in torch ops: s [N][C], one softmax per graph and channel"""
    m = torch.full((G, s.shape[1]), float("-inf"), device=s.device).scatter_reduce(0, gi[:, None].expand_as(s), s, "amax")
    p = torch.exp(s - m.detach()[gi])
    return p / torch.zeros((G, s.shape[1]), device=s.device).index_add(0, gi, p)[gi]


def set2set_torch(x, gi, G, Wi, Wh, b):
    z = lambda: torch.zeros((G, D), device=x.device)      # noqa: E731
    q, r, h, c = z(), z(), z(), z()
    for _ in range(ITERS):
        a = torch.cat([q, r], dim=1) @ Wi.T + h @ Wh.T + b
        i, f, gg, o = a.chunk(4, dim=1)
        c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(gg)
        h = torch.sigmoid(o) * torch.tanh(c)
        q = h
        alpha = segment_softmax((x * q[gi]).sum(dim=1, keepdim=True), gi, G)
        r = torch.zeros((G, D), device=x.device).index_add(0, gi, alpha * x)
    return torch.cat([q, r], dim=1)


def gap_torch(x, gi, G, fgate, ffeat):
    gate = x @ fgate.weight.T + fgate.bias
    feats = torch.relu(x @ ffeat.weight.T + ffeat.bias)
    return torch.zeros((G, D), device=x.device).index_add(0, gi, segment_softmax(gate, gi, G) * feats)


def shape_entries(tag, g, gen):
    """[(name, fn)] of one shape, and the worst norm-wise distances met while checking them at the timed size"""
    N, G = g.num_nodes, g.num_graphs
    gi = (g.graph_indicator - g.index_base).long()
    rnd = lambda *shape: (torch.rand(shape, generator=gen) - 0.5).cuda()      # noqa: E731
    x, d2, d1 = rnd(N, D), rnd(G, 2 * D), rnd(G, D)
    s2s = gnnmp.Set2Set(D, ITERS, seed=7)
    s2s.b = 0.1 * rnd(4 * D)
    fgate, ffeat = gnnmp.Dense((D, 1), seed=8), gnnmp.Dense((D, D), "relu", seed=9)
    gap = GlobalAttentionPool(fgate, ffeat)
    xg = x.clone().requires_grad_(True)
    ps_s, ps_g = [s2s.Wi, s2s.Wh, s2s.b], [fgate.weight, fgate.bias, ffeat.weight, ffeat.bias]
    rel = lambda a, b: float((a.double() - b.double()).norm() / b.double().norm())      # noqa: E731

    def no_grad(fn, *a):
        def run():
            with torch.no_grad():
                return fn(*a)
        return run

    def train(fn, leaves, dout):
        def run():
            for v in leaves:
                v.grad = None
            out = fn()
            out.backward(dout)
            return out
        return run
    s2s_forward, s2s_fused = no_grad(gnnmp.set2set_pool, s2s, g, x), no_grad(gnnmp.set2set_ad, s2s, g, x)
    gap_forward, gap_fused = no_grad(gnnmp.global_attention_pool, gap, g, x), no_grad(gnnmp.global_attention_pool_ad, gap, g, x)
    fwd = max(rel(s2s_fused(), s2s_forward()), rel(gap_fused(), gap_forward()))
    assert fwd <= 1e-4, f"{tag}: a fused forward differs from the existing one by {fwd:.2e} norm-wise"
    for p in ps_s + ps_g:
        p.requires_grad_(True)
    s2s_train = train(lambda: gnnmp.set2set_ad(s2s, g, xg), [xg] + ps_s, d2)
    s2s_torch = train(lambda: set2set_torch(xg, gi, G, s2s.Wi, s2s.Wh, s2s.b), [xg] + ps_s, d2)
    gap_train = train(lambda: gnnmp.global_attention_pool_ad(gap, g, xg), [xg] + ps_g, d1)
    gap_ttrain = train(lambda: gap_torch(xg, gi, G, fgate, ffeat), [xg] + ps_g, d1)
    grads = 0.0
    # (the gate's one bias shifts every logit of a softmax alike: its gradient is zero but for rounding, and is left out of the comparison)
    for ours, theirs, leaves in ((s2s_train, s2s_torch, [xg] + ps_s), (gap_train, gap_ttrain, [xg, fgate.weight, ffeat.weight, ffeat.bias])):
        ours()
        mine = [v.grad.clone() for v in leaves]
        theirs()
        grads = max([grads] + [rel(a, v.grad) for a, v in zip(mine, leaves)])
    assert grads <= 1e-3, f"{tag}: a gradient differs from torch autograd's by {grads:.2e} norm-wise"
    entries = [("s2s_forward", s2s_forward), ("s2s_fused_forward", s2s_fused), ("s2s_train", s2s_train), ("s2s_torch_train", s2s_torch),
               ("gap_forward", gap_forward), ("gap_fused_forward", gap_fused), ("gap_train", gap_train), ("gap_torch_train", gap_ttrain)]
    return [(f"{tag}.{k}", fn) for k, fn in entries], fwd, grads


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_readout needs a GPU: nothing is measured without one")
    gen = torch.Generator(device="cpu").manual_seed(1)
    qm9 = gnnmp.batch_arrays(synth.batched_graphs(G=4096, nmin=9, nmax=29, deg=2, seed=3))
    clouds, points = 32, 1024
    one = torch.zeros(1, dtype=torch.int64, device="cuda")
    cl = gnnmp.GNNGraph(one, one + 1, num_nodes=clouds * points, graph_indicator=torch.arange(clouds).repeat_interleave(points).cuda(),
                        num_graphs=clouds, index_base=0)
    entries, fwd, grads = [], 0.0, 0.0
    for tag, g in (("qm9", qm9), ("clouds", cl)):
        e, f, gr = shape_entries(tag, g, gen)
        entries, fwd, grads = entries + e, max(fwd, f), max(grads, gr)
    rounds = []
    for _ in range(args.rounds):
        rounds.append({name: timed(fn, args.reps, args.warmup) for name, fn in entries})
    ms = {k: min(r[k] for r in rounds) for k in rounds[0]}
    ratios = {}
    for tag in ("qm9", "clouds"):
        for kind in ("s2s", "gap"):
            ratios[f"{tag}.{kind}_forward_over_fused"] = ms[f"{tag}.{kind}_forward"] / ms[f"{tag}.{kind}_fused_forward"]
            ratios[f"{tag}.{kind}_torch_train_over_train"] = ms[f"{tag}.{kind}_torch_train"] / ms[f"{tag}.{kind}_train"]
    print(json.dumps({"tool": "bench_readout", "device": torch.cuda.get_device_name(0), "reps": args.reps, "rounds": args.rounds,
                      "channels": D, "set2set_iters": ITERS, "qm9": {"G": qm9.num_graphs, "N": qm9.num_nodes},
                      "clouds": {"G": clouds, "N": clouds * points}, "ms_per_round": rounds, "ms": ms, "ratios": ratios,
                      "worst_rel_between_forwards": fwd, "worst_rel_against_torch_autograd": grads}))


if __name__ == "__main__":
    main()
