"""EvolveGCNO timing: the layer (T launches of the batch-one LSTM step kernel, one propagate over the block-diagonal batch of the
snapshots, one dense a snapshot) against two comparators, back to back in one process.
    forward                  layer(tg, xs) under torch.no_grad()
    forward_composed         the same layer step by step from what existed before: gnnmp.dense at N = 1 twice, gnnmp_lstm_pointwise_f32,
                             gcn_conv(conv_weight = W_t) a snapshot                                                          yardstick
    forward_torch_lstm       the LSTM in torch ops (torch.addmv: rocBLAS gemv; torch elementwise), the convolutions as in the layer   yardstick
    train                    evolve_gcno_ad + the gradients of every x_t and every parameter
    lstm_train               the LSTM alone, forward and pullback: evolve_weights + lstm_pullback, given cotangents for every W_t
    lstm_train_torch         the same in torch ops under torch autograd                                                      yardstick
    step_kernel              gnnmp_lstm_matvec_cell_f32 alone; step_TBps = 8 D^2 4 bytes over its time
    step_kernel_one_wave     the same with the lane group pinned to one wave (knob 1): what D <= 2048 would run without the workgroup-wide
                             group; two host calls of gnnmp_tune are inside its time
Workload: T = 12 snapshots of about 6 000 nodes (5 700 .. 6 300), in-degree about 6; --ch 32 (D = 1024: 32 MB of LSTM weights, cache
resident) and --ch 64 (D = 4096: 512 MB, HBM).  Device events after --warmup calls, median of --reps and the spread (min, max) of every
round; rounds alternate the entries.  Before timing the three forwards are compared (norm-wise).  Prints ONE JSON line a channel count.
    python tools/bench_evolve_gcno.py [--ch 32 64] [--reps 10] [--warmup 3] [--rounds 2] [--T 12] [--nodes 6000]"""
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
from gnnmp.backward_evolve import lstm_pullback  # noqa: E402
from gnnmp.layers_temporal import evolve_conv, evolve_weights  # noqa: E402


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
    return [round(float(np.median(ts)), 4), round(float(min(ts)), 4), round(float(max(ts)), 4)]


def snapshots(T, nodes, deg, seed):
    rng = np.random.default_rng(seed)
    gs = []
    for k in range(T):
        n = int(nodes * (0.95 + 0.1 * rng.random()))
        s, t = rng.integers(1, n + 1, n * deg), rng.integers(1, n + 1, n * deg)
        gs.append(gnnmp.GNNGraph(torch.from_numpy(s).cuda(), torch.from_numpy(t).cuda(), num_nodes=n))
    return gnnmp.TemporalSnapshotsGNNGraph(gs)


def torch_lstm(cell, T, w=None):
    """the weight sequence in torch ops: [T][D]"""
    l = cell.lstm
    w = cell.conv.weight.t().reshape(-1) if w is None else w
    D = w.numel()
    h, c = torch.zeros_like(w), torch.zeros_like(w)
    out = []
    for _ in range(T):
        a = torch.addmv(torch.addmv(l.b, l.Wi, w), l.Wh, h)
        c = torch.sigmoid(a[D:2 * D]) * c + torch.sigmoid(a[:D]) * torch.tanh(a[2 * D:3 * D])
        h = torch.sigmoid(a[3 * D:]) * torch.tanh(c)
        w = h
        out.append(h)
    return torch.stack(out)


def composed(cell, tg, xs):
    """the layer step by step from the exports that existed before csrc/evolve.hip"""
    l, lib = cell.lstm, L.load()
    D = cell.in_ * cell.out
    w = cell.conv.weight.t().reshape(1, D).contiguous()
    h, c = torch.zeros_like(w), torch.zeros_like(w)
    ys = []
    for g, x in zip(tg, xs):
        gx, gh = gnnmp.dense(w, l.Wi), gnnmp.dense(h, l.Wh)
        hn, cn = torch.empty_like(h), torch.empty_like(c)
        L.check(lib.gnnmp_lstm_pointwise_f32(L.ptr(gx), L.ptr(gh), L.ptr(l.b), L.ptr(c), L.ptr(hn), L.ptr(cn), 1, D, L.stream_ptr()))
        w = h = hn
        c = cn
        ys.append(gnnmp.gcn_conv(cell.conv, g, x, conv_weight=h.view(cell.in_, cell.out).t().contiguous()))
    return ys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ch", type=int, nargs="+", default=[32, 64])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--T", type=int, default=12)
    ap.add_argument("--nodes", type=int, default=6000)
    a = ap.parse_args()
    tg = snapshots(a.T, a.nodes, 6, seed=1)
    gen = torch.Generator().manual_seed(0)
    for ch in a.ch:
        D = ch * ch
        layer = gnnmp.EvolveGCNO((ch, ch), seed=3)
        cell = layer.cell
        cell.lstm.b = ((torch.rand(4 * D, generator=gen) - 0.5)).cuda()
        xs = [(torch.rand((n, ch), generator=gen) - 0.5).cuda() for n in tg.num_nodes]
        dys = [(torch.rand((n, ch), generator=gen) - 0.5).cuda() for n in tg.num_nodes]
        dM = [(torch.rand(D, generator=gen) - 0.5).cuda() for _ in range(a.T)]
        params = [p.requires_grad_() for p in cell.parameters()]
        xcat = torch.cat(xs)

        def fwd():
            with torch.no_grad():
                return layer(tg, xs)

        def fwd_c():
            with torch.no_grad():
                return composed(cell, tg, xs)

        def fwd_t():
            with torch.no_grad():
                W = torch_lstm(cell, a.T)
                return evolve_conv(cell, tg, xcat, torch.cat([W[:1], W]))[0]

        def train():
            xd = [x.detach().requires_grad_() for x in xs]
            return torch.autograd.grad(gnnmp.evolve_gcno_ad(layer, tg, xd), xd + params, dys)

        def lstm_train():
            with torch.no_grad():
                Wseq, Cseq, A = evolve_weights(cell, a.T, None, None, None, keep=True)
                return lstm_pullback(cell, Wseq, Cseq, A, dM, None)

        def lstm_train_t():
            W = torch_lstm(cell, a.T)
            return torch.autograd.grad(W, [params[0], params[2], params[3], params[4]], torch.stack(dM))
        job_bufs = [torch.empty(D, device="cuda") for _ in range(2)] + [torch.rand(D, device="cuda") - 0.5 for _ in range(3)]
        job = L.LstmMatvecJob(L.ptr(cell.lstm.Wi), L.ptr(cell.lstm.Wh), L.ptr(job_bufs[2]), L.ptr(job_bufs[3]), L.ptr(job_bufs[4]),
                              L.ptr(cell.lstm.b), L.ptr(job_bufs[0]), L.ptr(job_bufs[1]), None)

        def step():
            L.check(L.load().gnnmp_lstm_matvec_cell_f32(ctypes.byref(job), D, L.stream_ptr()))

        def step_one_wave():                                 # the same kernel with one wave an element at every D (knob 1 pins the group)
            with L.tuned(L.Knob.FORCE_LOG2G, 6):
                step()
        u, w = torch.cat(fwd()), fwd_t()
        try:
            v, composed_error = torch.cat(fwd_c()), None
        except gnnmp.GnnmpError as e:                          # what exists has no route for this shape: say so, time the rest
            v, composed_error = u, str(e)
        g_new, g_t = lstm_train(), lstm_train_t()
        res = {"bench": "evolve_gcno", "device": torch.cuda.get_device_name(0), "in": ch, "out": ch, "D": D, "T": a.T,
               "nodes": sum(tg.num_nodes), "edges": sum(tg.num_edges), "lstm_weight_MB": round(8 * D * D * 4 / 2 ** 20, 1),
               "forward_rel_diff": {"composed": float((u - v).norm() / v.norm()), "torch_lstm": float((u - w).norm() / w.norm())},
               "lstm_grad_rel_diff": {"Wi": float((g_new[3] - g_t[1]).norm() / g_t[1].norm()), "Wh": float((g_new[4] - g_t[2]).norm() / g_t[2].norm())},
               "ms": {}}
        entries = [("forward", fwd), ("forward_composed", fwd_c), ("forward_torch_lstm", fwd_t), ("train", train), ("lstm_train", lstm_train),
                   ("lstm_train_torch", lstm_train_t), ("step_kernel", step), ("step_kernel_one_wave", step_one_wave)]
        if composed_error is not None:
            res["forward_composed_error"] = composed_error
            entries = [e for e in entries if e[0] != "forward_composed"]
        for name, _ in entries:
            res["ms"][name] = []
        for _ in range(a.rounds):
            for name, fn in entries:
                res["ms"][name].append(timed(fn, a.reps, a.warmup))
        res["step_TBps"] = [round(8 * D * D * 4 / (m[0] * 1e-3) / 1e12, 3) for m in res["ms"]["step_kernel"]]
        print(json.dumps(res), flush=True)
        del layer, cell, params


if __name__ == "__main__":
    main()
