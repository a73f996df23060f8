"""Heterograph attention timing: HeteroGraphConv of GATConv / GATv2Conv members through ONE hetero_attn_kernel launch per layer
(csrc/hetero_attn.hip) against the composition it replaces — the one-pass attention kernel per relation, then the identity-relation
combiner (knob 22 < 0) — on the same device, in one process, A, B, A, B.  Per shape:
    forward    model(g, x): the fused launch against the composition (the dense projections are in both)
    train      hetero_conv_ad forward + backward (sum of the outputs as the loss): the fused forward with statistics against the
               per-relation forwards; the pullback is per relation in both
    kernel     the attention part alone: gnnmp_hetero_attn_f32 on ready projections against gnnmp_gat_conv_f32 / gnnmp_attn_conv_f32 per
               relation + the combiner (and, on the hub shape, the fused kernel FORCED over the hub row: one lane group walks it whole)
Shapes:
    three_types   users, items, tags (200 k, 100 k, 20 k nodes); six relations of 0.2 M .. 2 M uniform random edges, no hubs
    hub           the same with one destination row of 50 k edges in one relation: the plan splits that row, so the layer sends its
                  destination type to the composition; `kernel_forced` shows what the whole-row walk would cost
Device events after warm-up, median of --reps.  Prints ONE JSON line.
    python tools/bench_hetero_attn.py [--reps 20] [--warmup 3] [--heads 4] [--out 16] [--din 64]"""
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
from gnnmp import hetero, hetero_attn  # noqa: E402


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


def ab(fused, composed, reps, warmup):
    """A, B, A, B: (fused ms, composed ms), each the better of its two medians"""
    def with_knob(fn):
        def run():
            L.tune(L.Knob.HETERO, -1)
            try:
                fn()
            finally:
                L.tune(L.Knob.HETERO, 0)
        return run
    a1 = timed(fused, reps, warmup)
    b1 = timed(with_knob(composed), reps, warmup)
    a2 = timed(fused, reps, warmup)
    b2 = timed(with_knob(composed), reps, warmup)
    return min(a1, a2), min(b1, b2)


def shape(name, seed=0):
    n = {"user": 200_000, "item": 100_000, "tag": 20_000}
    m = {("user", "rates", "item"): 2_000_000, ("item", "rated_by", "user"): 2_000_000, ("user", "follows", "user"): 1_000_000,
         ("tag", "labels", "item"): 500_000, ("item", "has", "tag"): 500_000, ("user", "uses", "tag"): 200_000}
    g = gnnmp.rand_heterograph(n, m, seed=seed)
    if name == "hub":
        et = ("user", "rates", "item")
        s, t = g.edge_index(et)
        t = t.clone()
        t[:50_000] = 7
        data = {e: g.edge_index(e) for e in g.etypes}
        data[et] = (s, t)
        g = gnnmp.GNNHeteroGraph(data, num_nodes=n)
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--heads", type=int, default=4)
    ap.add_argument("--out", type=int, default=16)
    ap.add_argument("--din", type=int, default=64)
    args = ap.parse_args()
    H, C, Din = args.heads, args.out, args.din
    out = {"tool": "bench_hetero_attn", "heads": H, "out": C, "din": Din, "reps": args.reps, "device": torch.cuda.get_device_name(0), "shapes": {}}
    for name in ("three_types", "hub"):
        g = shape(name)
        gen = torch.Generator(device="cpu").manual_seed(1)
        x = {nt: torch.rand((n, Din), generator=gen).cuda() for nt, n in g.num_nodes.items()}
        make = lambda k: (gnnmp.GATConv if k % 2 == 0 else gnnmp.GATv2Conv)((Din, C), heads=H, add_self_loops=False, seed=k)      # noqa: E731
        model = gnnmp.HeteroGraphConv({et: make(k) for k, et in enumerate(g.etypes)})
        rec = {"edges": int(sum(g.num_edges.values())), "relations": len(g.etypes), "split_rows": int(sum(g.plan(et).n_long for et in g.etypes))}
        f, c = ab(lambda: model(g, x), lambda: model(g, x), args.reps, args.warmup)
        rec["forward_ms"] = {"auto": f, "composition": c}

        names = lambda l: ("dense_x_weight", "a", "bias") if isinstance(l, gnnmp.GATConv) else ("dense_i_weight", "dense_i_bias", "dense_j_weight", "a", "bias")      # noqa: E731
        params = [getattr(l, n).requires_grad_() for l in model.layers for n in names(l)]
        xg = {k: v.clone().requires_grad_() for k, v in x.items()}

        def train():
            y = gnnmp.hetero_conv_ad(model, g, xg)
            torch.autograd.grad(sum(v.sum() for v in y.values()), list(xg.values()) + params)
        f, c = ab(train, train, args.reps, args.warmup)
        rec["train_ms"] = {"auto": f, "composition": c}

        # the attention part alone, on ready projections
        proj = hetero_attn.Projections(x)
        by_dst = {}
        for et, l in zip(model.etypes, model.layers):
            by_dst.setdefault(et[2], []).append((et, l))
        ops = {et: hetero_attn.relation_operands(l, et, proj) for et, l in zip(model.etypes, model.layers)}
        outs = {t: torch.empty((g.num_nodes[t], H * C), device="cuda") for t in by_dst}
        recs = [(outs[t], g.num_nodes[t], L.SUM, [(g.plan(et), *ops[et], l.bias, None, l.negative_slope, L.ACT_IDENTITY) for et, l in ms])
                for t, ms in by_dst.items()]
        lib = L.load()

        def per_relation():
            ys = {}
            for t, ms in by_dst.items():
                ys[t] = []
                for et, l in ms:
                    mode, Q, K, a = ops[et]
                    y = torch.empty((g.num_nodes[t], H * C), device="cuda")
                    if mode == hetero_attn.ATTN_GAT:
                        L.check(lib.gnnmp_gat_conv_f32(g.plan(et).handle, L.ptr(K), None if Q is K else L.ptr(Q), L.ptr(a), float(l.negative_slope),
                                                       L.ptr(l.bias), L.ACT_IDENTITY, L.ptr(y), H, C, L.stream_ptr()))
                    else:
                        L.check(lib.gnnmp_attn_conv_f32(g.plan(et).handle, mode, L.ptr(Q), L.ptr(K), None, L.ptr(a), float(l.negative_slope), 1.0,
                                                        L.ptr(l.bias), L.ACT_IDENTITY, L.ptr(y), None, H, C, L.stream_ptr()))
                    ys[t].append(y)
            hetero._combine(ys, L.SUM, H * C)
        fused_kernel = timed(lambda: hetero_attn.hetero_attn_call(recs, H, C), args.reps, args.warmup)
        rec["kernel_ms"] = {("kernel_forced" if rec["split_rows"] else "fused"): fused_kernel, "per_relation": timed(per_relation, args.reps, args.warmup)}
        out["shapes"][name] = rec
    print(json.dumps(out))


if __name__ == "__main__":
    main()
