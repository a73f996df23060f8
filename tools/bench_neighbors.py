"""Neighbour-search timing: gnnmp.knn_graph against what a user could do before it existed, on the same device — torch.cdist +
torch.topk (padded-batched over the clouds) followed by GNNGraph(s, t) with its plan build (gnnmp_plan_create: a sort).  Shapes:
    modelnet   32 clouds x 1024 points, d = 3,  k = 20   (a ModelNet batch)
    dgcnn      32 clouds x 1024 points, d = 64, k = 20   (a DGCNN inner layer: the graph is rebuilt from the features)
    cloud64k   1 cloud of 65 536 points, d = 3, k = 16
Reported per shape: graph + plan (gnnmp_knn_graph_f32, whose result IS the plan, + gnnmp_plan_edge_index into preallocated (s, t);
for the baseline cdist + topk + index arithmetic + GNNGraph's plan build), the baseline's search without its plan build, and
time-to-first-propagate (graph + plan + one propagate(copy_xj, max)); A, B, A, B in one process, device events after warm-up, median of
--reps.  The call builds a plan (allocations, one synchronisation), so its time is an UPPER bound of the search kernel's; pair
evaluations per second and the share of the fp32 vector peak (3 d flops a pair: sub, fma; peak = 256 CUs x 4 SIMDs x 32 lanes x
2 flop x 2.4 GHz = 157 Tflop/s) are computed from it and are lower bounds.  Prints ONE JSON line.
    python tools/bench_neighbors.py [--reps 20] [--warmup 3]"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graphneuralnetworks.jl_amd"))

import gnnmp  # noqa: E402
from gnnmp import _lib as L  # noqa: E402

PEAK_FP32 = 256 * 4 * 32 * 2 * 2.4e9
SHAPES = (("modelnet", 32, 1024, 3, 20), ("dgcnn", 32, 1024, 64, 20), ("cloud64k", 1, 65536, 3, 16))


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


def torch_knn(x, B, n, k):
    """(s, t) 1-based, destination-major like knn_graph(dir = :in), no self loops: cdist + topk per cloud, batched"""
    xb = x.view(B, n, -1)
    dist = torch.cdist(xb, xb)
    dist.diagonal(dim1=1, dim2=2).fill_(float("inf"))
    rows = 4096                                                   # topk over row blocks keeps the index temporaries bounded
    nb = torch.cat([dist[:, r0:r0 + rows].topk(k, dim=2, largest=False).indices for r0 in range(0, n, rows)], dim=1)
    off = (torch.arange(B, device=x.device) * n).view(B, 1, 1)
    s = (nb + off).reshape(-1) + 1
    t = torch.arange(B * n, device=x.device).repeat_interleave(k) + 1
    return s, t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default="modelnet,dgcnn,cloud64k")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_neighbors needs the GPU: there is no CPU fallback and no CPU timing"
    lib = L.load()
    out = {"bench": "neighbors", "reps": a.reps, "shapes": {}}
    for name, B, n, d, k in SHAPES:
        if name not in a.shapes.split(","):
            continue
        N = B * n
        gen = torch.Generator(device="cuda").manual_seed(7)
        x = torch.rand((N, d), device="cuda", generator=gen)
        gi = (torch.arange(N, device="cuda") // n + 1) if B > 1 else None
        feats = torch.randn((N, 64), device="cuda", generator=gen)
        s = torch.empty(N * k, dtype=torch.int64, device="cuda")
        t = torch.empty_like(s)

        def ours_search():
            h = ctypes.c_void_p()
            L.check(lib.gnnmp_knn_graph_f32(ctypes.byref(h), L.ptr(x), N, d, k, L.ptr(gi), 8, 1, B, 0, L.stream_ptr()))
            L.check(lib.gnnmp_plan_edge_index(h, 8, 1, L.ptr(s), L.ptr(t), L.stream_ptr()))
            L.check(lib.gnnmp_plan_destroy(h))

        def ours_first():
            g = gnnmp.knn_graph(x, k, gi)
            return gnnmp.propagate(gnnmp.copy_xj, g, "max", xj=feats)

        def base_search():
            return torch_knn(x, B, n, k)

        def base_graph():
            bs, bt = torch_knn(x, B, n, k)
            gnnmp.GNNGraph(bs, bt, num_nodes=N, graph_indicator=gi, num_graphs=B, _validated=True).plan(False)

        def base_first():
            bs, bt = torch_knn(x, B, n, k)
            g = gnnmp.GNNGraph(bs, bt, num_nodes=N, graph_indicator=gi, num_graphs=B, _validated=True)
            return gnnmp.propagate(gnnmp.copy_xj, g, "max", xj=feats)

        row = {"B": B, "n": n, "d": d, "k": k}
        for rnd in range(2):                                      # A, B, A, B: the spread between the rounds is the box noise
            for key, fn in (("ours_graph_ms", ours_search), ("torch_graph_ms", base_graph), ("torch_search_ms", base_search), ("ours_first_ms", ours_first),
                            ("torch_first_ms", base_first)):
                row.setdefault(key, []).append(timed(fn, a.reps, a.warmup))
        # the two agree up to the tie band (cdist's sqrt / matmul form): the share of equal neighbour sets
        g = gnnmp.knn_graph(x, k, gi)
        bs, _ = torch_knn(x, B, n, k)
        row["same_sets"] = float((torch.sort(g.s.view(N, k), dim=1)[0] == torch.sort(bs.view(N, k), dim=1)[0]).all(dim=1).float().mean())
        pairs = float(B) * n * n
        best = min(row["ours_graph_ms"]) * 1e-3
        row["pairs_per_s"] = pairs / best
        row["share_of_fp32_peak"] = pairs * 3 * d / best / PEAK_FP32
        row["graph_speedup"] = min(row["torch_graph_ms"]) / min(row["ours_graph_ms"])
        row["first_propagate_speedup"] = min(row["torch_first_ms"]) / min(row["ours_first_ms"])
        out["shapes"][name] = row
    print(json.dumps(out))


if __name__ == "__main__":
    main()
