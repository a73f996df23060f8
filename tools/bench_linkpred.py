"""Link-prediction timing (examples/link_prediction_pubmed.jl on the library's kernels): negative_sample at the PubMed shape (n = 19 717,
E = 88 648, bidirected) and at the ogbn-products shape (n = 2 449 029, E = 123 718 280 random edges, num_neg = E), rand_edge_split(0.9)
at the PubMed shape, one training step of the example's model (GCNConv(500 => 64, relu), GCNConv(64 => 64), DotDecoder on the positive
and a freshly sampled negative graph, logit BCE, backward), and the fused edge-dot adjoint (alias mode, D = 64) against the composition
of two propagates (knob 21 < 0), back to back, at both shapes.  Device-event timing after warm-up (median of --reps); prints ONE JSON line.
    python tools/bench_linkpred.py [--reps 20] [--warmup 3] [--no-products]"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graphneuralnetworks.jl_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import gnnmp  # noqa: E402
from gnnmp import _lib  # noqa: E402
from gnnmp.backward import gcn_conv_ad  # noqa: E402
from test_linkpred import planted_links  # noqa: E402


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


def adjoint_ab(g, D, reps, warmup):
    """fused alias-mode adjoint vs the two-propagate composition, alternated in one process"""
    gen = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn((g.num_nodes, D), device="cuda", generator=gen)
    dz = torch.randn(g.num_edges, device="cuda", generator=gen)
    g.plan(False), g.plan_transposed(False)
    fn = lambda: gnnmp.edge_dot_grad(g, x, x, dz, alias=True)
    row = {}
    outs = {}
    for rnd in range(2):                      # A, B, A, B: the spread between rounds is the box noise
        for path, kv in (("fused", 0), ("composed", -1)):
            _lib.tune(_lib.Knob.EDGE_DOT_GRAD, kv)
            try:
                row.setdefault(path + "_ms", []).append(timed(fn, reps, warmup))
                outs[path] = fn()[0]
            finally:
                _lib.tune(_lib.Knob.EDGE_DOT_GRAD, 0)
    row["max_rel_diff"] = float((outs["fused"] - outs["composed"]).abs().max() / outs["composed"].abs().max().clamp(min=1e-30))
    row["speedup"] = min(row["composed_ms"]) / min(row["fused_ms"])
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-products", action="store_true")
    a = ap.parse_args()
    res = {"bench": "linkpred", "device": torch.cuda.get_device_name(0)}

    # PubMed shape
    s, t, x = planted_links()
    n, D = x.shape
    g = gnnmp.GNNGraph(torch.from_numpy(s).cuda(), torch.from_numpy(t).cuda(), num_nodes=n)
    X = torch.from_numpy(x).cuda()
    pub = {"n": n, "E": g.num_edges, "D": D}
    pub["negative_sample_ms"] = timed(lambda: gnnmp.negative_sample(g, bidirected=True), a.reps, a.warmup)
    pub["rand_edge_split_ms"] = timed(lambda: gnnmp.rand_edge_split(g, 0.9, bidirected=True), a.reps, a.warmup)
    train_pos, _ = gnnmp.rand_edge_split(g, 0.9, bidirected=True, seed=17)
    l1, l2 = gnnmp.GCNConv((D, 64), "relu", seed=1), gnnmp.GCNConv((64, 64), None, seed=2)
    params = [l1.weight, l1.bias, l2.weight, l2.bias]
    for p in params:
        p.requires_grad_(True)
    opt = torch.optim.Adam(params, lr=1e-3)
    parts = {}

    def step(probe=False):
        opt.zero_grad()
        h = gcn_conv_ad(l2, train_pos, gcn_conv_ad(l1, train_pos, X))
        e0 = torch.cuda.Event(enable_timing=True)
        e0.record()
        neg = gnnmp.negative_sample(train_pos, bidirected=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e1.record()
        ps, ns = gnnmp.dot_decoder_ad(train_pos, h)[:, 0], gnnmp.dot_decoder_ad(neg, h)[:, 0]   # (neg's plans are built here)
        e2 = torch.cuda.Event(enable_timing=True)
        e2.record()
        scores = torch.cat([ps, ns])
        loss = F.binary_cross_entropy_with_logits(scores, torch.cat([torch.ones_like(ps), torch.zeros_like(ns)]))
        loss.backward()
        opt.step()
        if probe:
            parts.setdefault("sample", []).append((e0, e1))
            parts.setdefault("decode_fwd_with_neg_plan", []).append((e1, e2))

    for rnd in range(2):                      # the step with the fused adjoint and with the composition, alternated
        for kv, name in ((0, "train_step_ms"), (-1, "train_step_composed_adjoint_ms")):
            _lib.tune(_lib.Knob.EDGE_DOT_GRAD, kv)
            try:
                pub.setdefault(name, []).append(timed(step, a.reps, a.warmup))
            finally:
                _lib.tune(_lib.Knob.EDGE_DOT_GRAD, 0)
    for _ in range(a.reps):
        step(probe=True)
    torch.cuda.synchronize()
    for k, v in parts.items():
        pub["train_step_" + k + "_ms"] = float(np.median([u.elapsed_time(w) for u, w in v]))
    pub["adjoint_D64"] = adjoint_ab(train_pos, 64, a.reps, a.warmup)
    res["pubmed"] = pub

    if not a.no_products:
        n, E = 2449029, 123718280
        gen = torch.Generator(device="cuda").manual_seed(7)
        s = torch.randint(1, n + 1, (E,), device="cuda", generator=gen, dtype=torch.int32)
        t = torch.randint(1, n + 1, (E,), device="cuda", generator=gen, dtype=torch.int32)
        gp = gnnmp.GNNGraph(s, t, num_nodes=n)
        del s, t
        prod = {"n": n, "E": E}
        prod["negative_sample_ms"] = timed(lambda: gnnmp.negative_sample(gp, num_neg_edges=E, bidirected=False), max(3, a.reps // 4), 1)
        prod["adjoint_D64"] = adjoint_ab(gp, 64, max(3, a.reps // 4), 1)
        res["products"] = prod
    print(json.dumps(res))


if __name__ == "__main__":
    main()
