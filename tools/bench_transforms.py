"""Edge-coalescing timing: gnnmp.to_bidirected and gnnmp.remove_multi_edges against what a user could do before they existed, on the
same device — the torch composition torch.unique(keys, return_inverse = True) + index_add_ (remove_multi_edges, `+`) or index_add_ and a
division by the counts (to_bidirected, `mean`) over the materialised [s; t], [t; s] list and the doubled edge data.  The two sides are
NOT bit-compatible: ours adds the copies of an edge in their stably sorted order (the reference's result), torch's index_add_ uses
floating-point atomics in no fixed order.  Edge list: products-shaped (N = 2 449 029 nodes, --edges directed edges, default 61 859 140,
heavy-tailed sources), a tenth of it repeated so that both transforms have something to merge; edge data of width D in {0, 1, 100}
(D = 0: indices only).  A, B, A, B in one process, device events after warm-up, median of --reps.  Every call includes its allocations
and, on our side, the host synchronisations of graph prep and the plan build of the coalescing.  Prints ONE JSON line.
    python tools/bench_transforms.py [--reps 5] [--warmup 1] [--edges 61859140]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graphneuralnetworks.jl_amd"))

import gnnmp  # noqa: E402

N_PRODUCTS, E_PRODUCTS = 2449029, 61859140


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


def edge_list(N, E, gen):
    """1-based (s, t): heavy-tailed sources, uniform targets, the last tenth a copy of the first"""
    m = E - E // 10
    s = (torch.rand(m, device="cuda", generator=gen) ** 3 * N).long().clamp_(0, N - 1) + 1
    t = torch.randint(1, N + 1, (m,), device="cuda", generator=gen)
    return torch.cat([s, s[:E - m]]), torch.cat([t, t[:E - m]])


def torch_coalesce(s, t, N, e, mirrored):
    """the composition: keys -> unique with inverse -> index_add_ (mean: divided by the counts); returns (s2, t2, e2)"""
    if mirrored:
        s, t = torch.cat([s, t]), torch.cat([t, s])
        e = None if e is None else torch.cat([e, e])
    keys = (s - 1) * N + (t - 1)
    uniq, inv = torch.unique(keys, return_inverse=True)
    s2, t2 = uniq // N + 1, uniq % N + 1
    if e is None:
        return s2, t2, None
    out = torch.zeros((uniq.numel(),) + tuple(e.shape[1:]), dtype=e.dtype, device=e.device)
    out.index_add_(0, inv, e)
    if mirrored:
        cnt = torch.zeros(uniq.numel(), dtype=e.dtype, device=e.device).index_add_(0, inv, torch.ones_like(inv, dtype=e.dtype))
        out /= cnt.view((-1,) + (1,) * (e.dim() - 1))
    return s2, t2, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--edges", type=int, default=E_PRODUCTS)
    ap.add_argument("--widths", default="0,1,100")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_transforms needs the GPU: there is no CPU fallback and no CPU timing"
    gen = torch.Generator(device="cuda").manual_seed(7)
    N, E = N_PRODUCTS, a.edges
    s, t = edge_list(N, E, gen)
    g = gnnmp.GNNGraph(s, t, num_nodes=N, _validated=True)
    out = {"bench": "transforms", "reps": a.reps, "N": N, "E": E, "rows": {}}
    for D in (int(v) for v in a.widths.split(",")):
        e = None if D == 0 else torch.randn((E, D), device="cuda", generator=gen)
        fns = {
            "to_bidirected": (lambda: gnnmp.to_bidirected(g, edata=e), lambda: torch_coalesce(s, t, N, e, True)),
            "remove_multi_edges": (lambda: gnnmp.remove_multi_edges(g, "+", edata=e), lambda: torch_coalesce(s, t, N, e, False)),
        }
        for name, (ours, base) in fns.items():
            row = {"D": D, "ours_ms": [], "torch_ms": []}
            for rnd in range(2):                                  # A, B, A, B: the spread between the rounds is the box noise
                row["ours_ms"].append(timed(ours, a.reps, a.warmup))
                row["torch_ms"].append(timed(base, a.reps, a.warmup))
            r = ours()
            g2 = r if e is None else r[0]
            row["edges_out"] = g2.num_edges
            row["same_edge_count"] = bool(g2.num_edges == base()[0].numel())
            row["torch_over_ours"] = min(row["torch_ms"]) / min(row["ours_ms"])
            out["rows"][f"{name}_D{D}"] = row
            del r, g2
        del e
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
