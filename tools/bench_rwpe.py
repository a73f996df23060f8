"""random_walk_pe timing: gnnmp.random_walk_pe against the reference's algorithm written in torch on the same device — RW = A * Diagonal(dinv)
as a sparse matrix, then either
  panels   RW @ panel for dense one-hot panels of --panel start nodes at a time (walk_length sparse x dense products a panel, the diagonal
           picked out of every product), which is what fits in memory at any size, or
  spgemm   the reference's own loop out = out * RW with torch.sparse.mm on two sparse matrices, where the fill-in fits (the batched shape
           only: a block-diagonal power stays block diagonal); recorded as "not available" when this torch build has no sparse x sparse
           product on the device.
Shapes: "zinc" — a batch of 10 000 molecule-sized graphs (about 23 nodes and 50 directed edges each), walk_length 20, all of it on the
LDS path; "single" — one unbatched graph of 20 000 nodes and 100 000 edges, walk_length 8, the scratch path.  A, B, A, B in one process,
device events after warm-up, median of --reps (ours: of at least 5 — a call is milliseconds, a panels run of the batched shape tens of
seconds, so that side is usually run with --reps 1 --warmup 0).  Ours is timed with the graph's transposed plan built (a constant of the
graph, like every plan); the first call, which builds it, is reported once as first_call_ms.  Prints ONE JSON line.
    python tools/bench_rwpe.py [--reps 3] [--warmup 1] [--shapes zinc,single] [--baselines panels,spgemm] [--panel 2048]"""
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


def zinc_batch(G, rng):
    """0-based (s, t, gi, N): every member a path over its nodes plus random chords, both directions, about 50 directed edges"""
    n = np.clip(np.rint(rng.normal(23.0, 4.0, G)), 9, 37).astype(np.int64)
    off = np.concatenate([[0], np.cumsum(n)])
    ss, tt = [], []
    for k in range(G):
        m = int(n[k])
        a = np.arange(m - 1)
        extra = max(0, int(round(m * 25 / 23)) - (m - 1))
        u, v = rng.integers(0, m, extra), rng.integers(0, m, extra)
        keep = u != v
        us, vs = np.concatenate([a, u[keep]]) + off[k], np.concatenate([a + 1, v[keep]]) + off[k]
        ss += [us, vs]
        tt += [vs, us]
    return np.concatenate(ss), np.concatenate(tt), np.repeat(np.arange(G), n), int(off[-1])


def torch_rw(s, t, N):
    """sparse RW = A * Diagonal(dinv), dinv from the out-degrees (row sums of A), coalesced"""
    A = torch.sparse_coo_tensor(torch.stack([s, t]), torch.ones(s.numel(), device=s.device), (N, N)).coalesce()
    deg = torch.zeros(N, device=s.device).index_add_(0, s, torch.ones(s.numel(), device=s.device))
    dinv = torch.where(deg > 0, 1.0 / deg, torch.zeros_like(deg))
    idx = A.indices()
    return torch.sparse_coo_tensor(idx, A.values() * dinv[idx[1]], (N, N)).coalesce()


def torch_panels(RW, N, K, panel):
    RWc = RW.to_sparse_csr()
    pe = torch.empty((N, K), device=RW.device)
    for c0 in range(0, N, panel):
        b = min(panel, N - c0)
        cols = torch.arange(b, device=RW.device)
        V = torch.zeros((N, b), device=RW.device)
        V[c0 + cols, cols] = 1.0
        for k in range(K):
            V = RWc @ V
            pe[c0:c0 + b, k] = V[c0 + cols, cols]
    return pe


def torch_spgemm(RW, N, K):
    pe = torch.zeros((N, K), device=RW.device)
    out = RW
    for k in range(K):
        if k > 0:
            out = torch.sparse.mm(out, RW).coalesce()
        idx = out.indices()
        d = idx[0] == idx[1]
        pe[idx[0][d], k] = out.values()[d]
    return pe


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--shapes", default="zinc,single")
    ap.add_argument("--panel", type=int, default=2048)
    ap.add_argument("--graphs", type=int, default=10000)
    ap.add_argument("--baselines", default="panels,spgemm")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_rwpe needs the GPU: there is no CPU fallback and no CPU timing"
    rng = np.random.default_rng(11)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    out = {"bench": "rwpe", "reps": a.reps, "panel": a.panel, "rows": {}}
    for shape in a.shapes.split(","):
        if shape == "zinc":
            s, t, gi, N = zinc_batch(a.graphs, rng)
            K, G = 20, a.graphs
            g = gnnmp.GNNGraph(dev(s + 1), dev(t + 1), num_nodes=N, graph_indicator=dev(gi + 1), num_graphs=G)
        else:
            N, E, K, G = 20000, 100000, 8, 1
            s, t = rng.integers(0, N, E), rng.integers(0, N, E)
            g = gnnmp.GNNGraph(dev(s + 1), dev(t + 1), num_nodes=N)
        sd, td = dev(s), dev(t)
        row = {"N": N, "E": int(len(s)), "graphs": G, "walk_length": K, "ours_ms": []}
        t0 = time.perf_counter()
        ours_pe = gnnmp.random_walk_pe(g, K)
        torch.cuda.synchronize()
        row["first_call_ms"] = (time.perf_counter() - t0) * 1e3
        RW = torch_rw(sd, td, N)
        ours = lambda: gnnmp.random_walk_pe(g, K)
        last = {}
        bases = {"panels": lambda: last.__setitem__("pe", torch_panels(RW, N, K, a.panel))}
        if shape == "zinc":
            bases["spgemm"] = lambda: last.__setitem__("pe", torch_spgemm(RW, N, K))
        for name in a.baselines.split(","):
            if name not in bases:
                continue
            key = f"torch_{name}_ms"
            row[key] = []
            try:
                for rnd in range(2):                          # A, B, A, B: the spread between the rounds is the box noise
                    row["ours_ms"].append(timed(ours, max(a.reps, 5), 1))
                    row[key].append(timed(bases[name], a.reps, a.warmup))
                row[f"max_abs_diff_{name}"] = float((ours_pe - last["pe"]).abs().max())
                row[f"{name}_over_ours"] = min(row[key]) / min(row["ours_ms"])
            except (RuntimeError, NotImplementedError) as e:
                row[key] = "not available: " + str(e).splitlines()[0][:120]
            last.clear()
        out["rows"][shape] = row
        del RW, g, ours_pe
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
