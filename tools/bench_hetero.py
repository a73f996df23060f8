"""Heterograph aggregation timing: ONE hetero_rows_kernel launch per layer (csrc/hetero.hip) against the composition it replaces — a
propagate per relation, then the same kernel over identity relations as the combiner (knob 22 < 0) — on the same device, in one
process, A, B, A, B.  Two layers of measurement per shape:
    aggregate   gnnmp.hetero_propagate(copy_xj, +) over the relations: the kernel against the composition
    layer       HeteroGraphConv of GraphConv(D => Dout, no activation): the transform-first fused path against the general path —
                this is the `Dout <= Din` gate of gnnmp/hetero.py, measured at Dout = D and Dout = D / 2
    backward    gnnmp.hetero_propagate_grad over the same relations, + and mean: ONE hetero_grad_rows_kernel launch for all source
                types (csrc/hetero_backward.hip) against the composition — a transposed propagate per relation, then the identity-relation
                sum (`--only backward` / `--only forward` run one half)
Shapes:
    few_large    2 node types, 3 relations of 2 M edges into 200 k rows each (users - items)
    many_small   1 destination type of 20 k rows with 12 incoming relations of 40 k edges, next to one of 2 M edges
    hub          few_large with one destination row of 50 k edges: the split-row fallback (the composition is what hetero_propagate
                 takes there; `kernel_forced` times the one-launch kernel walking the hub with one lane group)
Device events after warm-up, median of --reps.  Algorithmic bytes: (4 D + 4) B per edge + 4 D B per destination row for the kernel, plus
2 * 4 D * R B per destination row for the composition.  Prints ONE JSON line.
    python tools/bench_hetero.py [--reps 20] [--warmup 3] [--D 128]"""
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
from gnnmp import hetero  # noqa: E402


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
    """{edge_t: (n_edges)} and node counts; edges uniform at random (host generator), the hub added by hand"""
    if name == "many_small":
        n = {"d": 20_000, **{f"s{k}": 5_000 for k in range(12)}, "big": 200_000}
        m = {(f"s{k}", "r", "d"): 40_000 for k in range(12)}
        m[("big", "r", "d")] = 2_000_000
        return gnnmp.rand_heterograph(n, m, seed=seed)
    n = {"user": 200_000, "item": 200_000}
    m = {("user", "rates", "item"): 2_000_000, ("item", "rated_by", "user"): 2_000_000, ("user", "follows", "user"): 2_000_000}
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
    ap.add_argument("--D", type=int, default=128)
    ap.add_argument("--only", choices=("forward", "backward"), default=None)
    args = ap.parse_args()
    D = args.D
    out = {"tool": "bench_hetero", "D": D, "reps": args.reps, "device": torch.cuda.get_device_name(0), "shapes": {}}
    for name in ("few_large", "many_small", "hub"):
        g = shape(name)
        gen = torch.Generator(device="cpu").manual_seed(1)
        x = {nt: torch.rand((n, D), generator=gen).cuda() for nt, n in g.num_nodes.items()}
        E = sum(g.num_edges.values())
        rows = {}
        for et in g.etypes:
            rows[et[2]] = rows.get(et[2], 0) + 1
        kernel_bytes = (4 * D + 4) * E + sum(4 * D * g.num_nodes[t] for t in rows)
        comp_bytes = kernel_bytes + sum(2 * 4 * D * r * g.num_nodes[t] for t, r in rows.items())
        rec = {"edges": E, "relations": len(g.etypes), "split_rows": int(sum(g.plan(et).n_long for et in g.etypes)),
               "kernel_algorithmic_MB": kernel_bytes / 1e6, "composition_algorithmic_MB": comp_bytes / 1e6}
        if args.only != "backward":
            run = lambda: gnnmp.hetero_propagate(g, x)      # noqa: E731
            f, c = ab(run, run, args.reps, args.warmup)
            rec["aggregate_ms"] = {"auto": f, "composition": c}
            if rec["split_rows"]:
                # the one-launch kernel walking the split rows whole (what the auto path avoids): called below the Python gate
                outs = {t: torch.empty((g.num_nodes[t], D), device="cuda") for t in rows}
                recs = [(outs[t], g.num_nodes[t], L.SUM, [(g.plan(et), x[et[0]], None, L.SUM) for et in g.etypes if et[2] == t]) for t in rows]
                rec["aggregate_ms"]["kernel_forced"] = timed(lambda: hetero._hetero_call(recs, D), args.reps, args.warmup)
            rec["aggregate_GBps"] = {"auto": kernel_bytes / f / 1e6, "composition": comp_bytes / c / 1e6}
            for Dout in (D, D // 2):
                model = gnnmp.HeteroGraphConv({et: gnnmp.GraphConv((D, Dout), seed=k) for k, et in enumerate(g.etypes)})
                run = lambda: model(g, x)                   # noqa: E731
                f, c = ab(run, run, args.reps, args.warmup)
                rec[f"layer_Dout{Dout}_ms"] = {"auto": f, "general": c}
        if args.only != "forward":
            # the adjoint w.r.t. x: Δ arrives at every destination type; a source row is finished over all its outgoing relations
            dy = {t: torch.rand((g.num_nodes[t], D), generator=gen).cuda() for t in rows}
            rec["split_rows_transposed"] = int(sum(g.plan(et, transposed=True).n_long for et in g.etypes))
            outgoing = {}
            for et in g.etypes:
                outgoing[et[0]] = outgoing.get(et[0], 0) + 1
            grad_bytes = (4 * D + 4) * E + sum(4 * D * g.num_nodes[s] for s in outgoing)
            for aggr in ("+", "mean"):
                run = lambda: gnnmp.hetero_propagate_grad(g, dy, aggr=aggr)      # noqa: E731
                f, c = ab(run, run, args.reps, args.warmup)
                rec[f"backward_{'sum' if aggr == '+' else aggr}_ms"] = {"auto": f, "composition": c}
            rec["backward_algorithmic_MB"] = grad_bytes / 1e6
        out["shapes"][name] = rec
    print(json.dumps(out))


if __name__ == "__main__":
    main()
