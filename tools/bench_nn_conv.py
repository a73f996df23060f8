"""NNConv's per-edge-matrix adjoint at a QM9-like shape: gnnmp_nn_conv_grad_f32 (csrc/nn_grad.hip: one walk of the transposed plan that
reads we once, writes dwe once and accumulates dx in registers) against a torch composition of the same two formulas on the same
device, in one process, alternating A, B, A, B.  Per in = out = D:
    A  export   gnnmp_nn_conv_grad_f32(plan_t, {x, we, dm, dx, dwe}, D, D)
    B  torch    dm.index_select(0, t), x.index_select(0, s); dwe = bmm(x_j [E][D][1], Δ_i [E][1][D]); dx = zeros.index_add_(0, s,
                bmm(we [E][D][D], Δ_i [E][D][1]))
Workload: a batch of small molecule-like graphs — 128 graphs x 18 points uniform in the unit cube, radius_graph per graph with a radius
that gives a mean degree of about 4 (reported, with the largest out-degree: the walk takes a source's row with one lane group).
Device events after --warmup calls, median of --reps, rounds alternate the two; every round is reported (a single run is a record, not a
claim).  For A also the algorithmic bytes — we read plus dwe written, 2 * E * D * D * 4 — per second.  Before timing, A is compared with B
at the timed size (norm-wise).  Prints ONE JSON line.
    python tools/bench_nn_conv.py [--reps 20] [--warmup 3] [--rounds 2] [--graphs 128] [--nodes 18] [--radius 0.47]"""
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

WIDTHS = (16, 32, 64)


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
    ap.add_argument("--graphs", type=int, default=128)
    ap.add_argument("--nodes", type=int, default=18)
    ap.add_argument("--radius", type=float, default=0.47)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_nn_conv needs a GPU: nothing is measured without one")
    gen = torch.Generator(device="cpu").manual_seed(1)
    N = args.graphs * args.nodes
    pos = torch.rand((N, 3), generator=gen).cuda()
    gi = torch.arange(args.graphs).repeat_interleave(args.nodes).cuda() + 1
    g = gnnmp.radius_graph(pos, args.radius, graph_indicator=gi)
    E = g.num_edges
    pt = g.plan_transposed(False)
    s0, t0 = g.s - 1, g.t - 1
    lib = L.load()
    out = {"tool": "bench_nn_conv", "device": torch.cuda.get_device_name(0), "reps": args.reps, "rounds": args.rounds, "N": N, "E": E,
           "mean_degree": E / N, "max_out_degree": int(pt.max_degree), "shapes": {}}
    for D in WIDTHS:
        x = (torch.rand((N, D), generator=gen) - 0.5).cuda()
        we = ((torch.rand((E, D * D), generator=gen) - 0.5) / D ** 0.5).cuda()
        dm = (torch.rand((N, D), generator=gen) - 0.5).cuda()
        dx, dwe = torch.empty_like(x), torch.empty_like(we)
        job = L.NNConvGradJob(L.ptr(x), L.ptr(we), L.ptr(dm), L.ptr(dx), L.ptr(dwe))

        def export():
            L.check(lib.gnnmp_nn_conv_grad_f32(pt.handle, ctypes.byref(job), D, D, L.stream_ptr()))
            return dx, dwe

        def composed():
            di, xj = dm.index_select(0, t0), x.index_select(0, s0)
            dwe_t = torch.bmm(xj.unsqueeze(2), di.unsqueeze(1)).view(E, D * D)          # [k][c][o]: element (o, c) at o + D c
            dx_t = torch.zeros((N, D), device="cuda").index_add_(0, s0, torch.bmm(we.view(E, D, D), di.unsqueeze(2)).squeeze(2))
            return dx_t, dwe_t

        rel = lambda a, b: float((a.double() - b.double()).norm() / b.double().norm())      # noqa: E731
        worst = max(rel(a, b) for a, b in zip(export(), composed()))
        assert worst <= 1e-5, f"D = {D}: the export differs from torch's float32 composition by {worst:.2e} norm-wise"
        rounds = []
        for _ in range(args.rounds):
            rounds.append({name: timed(fn, args.reps, args.warmup) for name, fn in (("export", export), ("torch", composed))})
        ms = {k: min(r[k] for r in rounds) for k in rounds[0]}
        nbytes = 2 * E * D * D * 4
        out["shapes"][f"in{D}_out{D}"] = {"ms_per_round": rounds, "ms": ms, "we_plus_dwe_bytes": nbytes,
                                          "export_GB_per_s": nbytes / (ms["export"] * 1e-3) / 1e9, "worst_rel_vs_torch_fp32": worst}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
