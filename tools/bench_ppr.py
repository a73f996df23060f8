"""ppr_diffusion timing: gnnmp.ppr_diffusion against what a user could do before on the same device — the reference's algorithm written in
torch: the dense matrix M = I + (alpha - 1) A by index_put_(accumulate), torch.linalg.inv, the inverse read back at the edges.  For one
graph that is the N x N matrix; for a batch a padded [G, n_max, n_max] stack of the member blocks (identity in the padding) through the
batched torch.linalg.inv, plus the index arithmetic from the node offsets (the baseline is given the offsets: they are a constant of the
batch on both sides).
Shapes: "zinc" — a batch of 10 000 molecule-sized graphs of about 23 nodes (LDS path); "b150" — a batch of 512 graphs of 150 nodes: in
LDS with the 160 KB budget the Python mirror asks for, and timed ALSO with lds_budget_bytes = 0, the C record's default of 64 KB (127
nodes), which sends every member through the scratch path one after another; "n1000", "n3000" — one graph of 1 000 / 3 000 nodes
(scratch path: two launches a pivot step).
A, B, A, B in one process, device events after warm-up, median of --reps.  Ours is timed with the graph's transposed plan and node
offsets built (constants of the graph); the first call, which builds them, is reported once as first_call_ms.  Prints ONE JSON line.
    python tools/bench_ppr.py [--reps 3] [--warmup 1] [--shapes zinc,b150,n1000,n3000]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graphneuralnetworks.jl_amd"))

import gnnmp  # noqa: E402

ALPHA = 0.85


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


def batch_of(sizes, per_node, rng):
    """0-based (s, t, w, off): every member a random multigraph of about per_node in-edges a node, weights in [0.1, 1]"""
    off = np.concatenate([[0], np.cumsum(sizes)])
    ss, tt = [], []
    for k, m in enumerate(sizes):
        E = int(m) * per_node
        ss.append(rng.integers(0, m, E) + off[k])
        tt.append(rng.integers(0, m, E) + off[k])
    s, t = np.concatenate(ss), np.concatenate(tt)
    return s, t, rng.uniform(0.1, 1.0, len(s)).astype(np.float32), off


def torch_single(s, t, w, N):
    M = torch.zeros((N, N), device=s.device)
    M.index_put_((t, s), (ALPHA - 1.0) * w, accumulate=True)
    M.diagonal().add_(1.0)
    return ALPHA * torch.linalg.inv(M)[t, s]


def torch_padded(s, t, w, off, gid):
    """off: int64 [G + 1] node offsets; gid: the member graph of every edge (computed once, like the offsets)"""
    G = off.numel() - 1
    nmax = int((off[1:] - off[:-1]).max())
    ls, lt = s - off[gid], t - off[gid]
    M = torch.zeros((G, nmax, nmax), device=s.device)
    M.index_put_((gid, lt, ls), (ALPHA - 1.0) * w, accumulate=True)
    M.diagonal(dim1=1, dim2=2).add_(1.0)
    return ALPHA * torch.linalg.inv(M)[gid, lt, ls]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--shapes", default="zinc,b150,n1000,n3000")
    ap.add_argument("--graphs", type=int, default=10000)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_ppr needs the GPU: there is no CPU fallback and no CPU timing"
    rng = np.random.default_rng(11)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    out = {"bench": "ppr", "reps": a.reps, "alpha": ALPHA, "rows": {}}
    for shape in a.shapes.split(","):
        if shape == "zinc":
            sizes = np.clip(np.rint(rng.normal(23.0, 4.0, a.graphs)), 9, 37).astype(np.int64)
            per_node = 2
        elif shape == "b150":
            sizes, per_node = np.full(512, 150, np.int64), 3
        else:
            sizes, per_node = np.array([int(shape[1:])], np.int64), 3
        s, t, w, off = batch_of(sizes, per_node, rng)
        G, N = len(sizes), int(off[-1])
        kw = {}
        if G > 1:
            kw = dict(graph_indicator=dev(np.repeat(np.arange(1, G + 1), sizes)), num_graphs=G)
        g = gnnmp.GNNGraph(dev(s + 1), dev(t + 1), dev(w), num_nodes=N, **kw)
        sd, td, wd, offd = dev(s), dev(t), dev(w), dev(off)
        gid = dev(np.repeat(np.arange(G), sizes * per_node))
        row = {"N": N, "E": int(len(s)), "graphs": G, "largest_member": int(sizes.max())}
        t0 = time.perf_counter()
        first = gnnmp.ppr_diffusion(g, ALPHA).w
        torch.cuda.synchronize()
        row["first_call_ms"] = (time.perf_counter() - t0) * 1e3
        sides = {"ours_ms": lambda: gnnmp.ppr_diffusion(g, ALPHA)}
        if shape == "b150":
            sides["ours_lds64k_scratch_ms"] = lambda: gnnmp.ppr_diffusion(g, ALPHA, lds_budget_bytes=0)
        last = {}
        if G > 1:
            sides["torch_padded_inv_ms"] = lambda: last.__setitem__("w", torch_padded(sd, td, wd, offd, gid))
        else:
            sides["torch_inv_ms"] = lambda: last.__setitem__("w", torch_single(sd, td, wd, N))
        for key in sides:
            row[key] = []
        for rnd in range(2):                                  # A, B, A, B: the spread between the rounds is the box noise
            for key, fn in sides.items():
                row[key].append(timed(fn, a.reps, a.warmup))
        row["max_abs_diff"] = float((first - last["w"]).abs().max())
        row["max_abs_w"] = float(first.abs().max())
        if shape == "b150":
            row["scratch_bit_identical"] = bool(torch.equal(first, gnnmp.ppr_diffusion(g, ALPHA, lds_budget_bytes=0).w))
        base = "torch_padded_inv_ms" if G > 1 else "torch_inv_ms"
        row["torch_over_ours"] = min(row[base]) / min(row["ours_ms"])
        out["rows"][shape] = row
        del g, first, last
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
