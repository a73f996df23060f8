"""Grouped dense against the per-segment loop it replaces (DESIGN.md §5 holds the table this prints).

    python tools/bench_grouped_dense.py [--reps 20] [--warmup 5] [--rounds 2] [--out FILE.json]

Entries of one shape alternate inside one process; a sample is device events around one call sequence (a loop of T launches is one
sample: the gain looked for is the launch count); the figure is the median of `reps` samples after `warmup`, per round.  Shapes:
  evolve   T = 12 snapshots of about 6 000 rows, 32 => 32 and 64 => 64: gnnmp_dense_f32 / gnnmp_dense_grad_w_f32 a snapshot vs one grouped call
  small    4 096 groups of 9 .. 29 rows, 64 => 64: the same
  long     4 groups of 300 000 rows, 128 => 128: the same — segments long enough for gnnmp_dense_f32's split-bf16 core to count
  layer    EvolveGCNO(8 => 8) over T = 12 snapshots of about 6 000 nodes, forward and a training step, grouped off and on
Needs a GPU: there is no other way to a time."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "graphneuralnetworks.jl_amd"))


def median_ms(entries, reps, warmup):
    """{name: median milliseconds}: the entries take turns, `warmup` untimed turns first"""
    import torch
    times = {k: [] for k in entries}
    for it in range(warmup + reps):
        for name, fn in entries.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if it >= warmup:
                times[name].append(e0.elapsed_time(e1))
    return {k: statistics.median(v) for k, v in times.items()}


def dense_entries(sizes, K, Dout):
    import torch
    import gnnmp
    from gnnmp.backward import dense_grad_w
    from gnnmp.grouped import grouped_grad_launch
    seg = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    N, G = int(seg[-1]), len(sizes)
    x, dz = torch.randn(N, K, device="cuda"), torch.randn(N, Dout, device="cuda")
    W = torch.randn(G, Dout, K, device="cuda")
    sp = torch.from_numpy(seg).cuda()
    out = torch.empty(N, Dout, device="cuda")
    dW = torch.empty(G, Dout, K, device="cuda")
    segl = seg.tolist()

    def loop_fwd():
        for g in range(G):
            if segl[g + 1] > segl[g]:
                gnnmp.dense(x[segl[g]:segl[g + 1]], W[g], out=out[segl[g]:segl[g + 1]])

    def loop_gradw():
        for g in range(G):
            if segl[g + 1] > segl[g]:
                dense_grad_w(dz[segl[g]:segl[g + 1]], x[segl[g]:segl[g + 1]], need_b=False)
    return {"loop forward": loop_fwd, "grouped forward": lambda: gnnmp.grouped_dense(x, W, sp),
            "loop grad_w": loop_gradw, "grouped grad_w": lambda: grouped_grad_launch(dz, Dout, x, K, sp, dW, Dout * K, None, 0, N, G, K, Dout)}


def layer_entries(T, n, ch):
    import torch
    import gnnmp
    rng = np.random.default_rng(1)
    snaps = []
    for _ in range(T):
        nt = n + int(rng.integers(-200, 201))
        s, t = rng.integers(1, nt + 1, 4 * nt), rng.integers(1, nt + 1, 4 * nt)
        snaps.append(gnnmp.GNNGraph(torch.from_numpy(s).cuda(), torch.from_numpy(t).cuda(), num_nodes=nt))
    tg = gnnmp.TemporalSnapshotsGNNGraph(snaps)
    xs = [torch.randn(g.num_nodes, ch[0], device="cuda") for g in snaps]
    entries = {}
    for grouped in (False, True):
        layer = gnnmp.EvolveGCNO(ch, seed=2, grouped=grouped)
        params = [p.requires_grad_() for p in layer.cell.parameters()]

        def train(layer=layer, params=params):
            ys = gnnmp.evolve_gcno_ad(layer, tg, xs)
            torch.autograd.grad(sum(y.sum() for y in ys), params)
        tag = "grouped" if grouped else "loop"
        entries[f"{tag} layer forward"] = lambda layer=layer: layer(tg, xs)
        entries[f"{tag} layer training"] = train
    return entries


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_grouped_dense needs a GPU"
    rng = np.random.default_rng(0)
    evolve = (6000 + rng.integers(-300, 301, 12)).tolist()
    small = rng.integers(9, 30, 4096).tolist()
    shapes = {"evolve T=12 x ~6000, 32=>32": lambda: dense_entries(evolve, 32, 32), "evolve T=12 x ~6000, 64=>64": lambda: dense_entries(evolve, 64, 64),
              "small 4096 x 9..29, 64=>64": lambda: dense_entries(small, 64, 64), "long 4 x 300000, 128=>128": lambda: dense_entries([300000] * 4, 128, 128),
              "EvolveGCNO 8=>8, T=12 x ~6000": lambda: layer_entries(12, 6000, (8, 8))}
    result = {}
    for shape, make in shapes.items():
        entries = make()
        heavy = shape.startswith("small")                       # 4 096 launches a sample: fewer samples say the same
        rounds = [median_ms(entries, max(3, a.reps // 4) if heavy else a.reps, 2 if heavy else a.warmup) for _ in range(a.rounds)]
        result[shape] = {k: [round(r[k], 4) for r in rounds] for k in entries}
        for k, v in result[shape].items():
            print(f"| {shape} | {k} | " + " | ".join(f"{t:.3f}" for t in v) + " |", flush=True)
    line = json.dumps({"bench": "grouped_dense", "unit": "ms", "median_of": a.reps, "rounds": a.rounds, "result": result})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
