"""GConvGRU, GConvLSTM and DCGRU timing: the layers (one x-side pass for all steps, per step one basis on panels -> one dense -> one gate
kernel) against each cell as the reference wrote it (temporalconv.jl:237-254, :416-437, :564-575), step by step on gnnmp.cheb_conv /
gnnmp.d_conv plus torch elementwise ops — and, for the training figure, torch autograd over gnnmp.cheb_conv_ad / gnnmp.d_conv_ad.
    <layer>_forward            layer(g, x) under torch.no_grad()
    <layer>_forward_composed   the composed cell scanned over T under torch.no_grad()                       the yardstick
    <layer>_train              <layer>_ad(layer, g, x) + gradients of x and every parameter
    <layer>_train_composed     the composed cell on the *_ad convolutions, torch autograd                   the yardstick
Workload: a batch of 64 road-like graphs (207 nodes, degree 8, bidirected, weighted), T = 12, in = 2, out = 64; Chebyshev K = 3,
diffusion k = 2.  Device events after --warmup calls, median of --reps, rounds alternate the entries; every round is reported (a single
run is a record, not a claim).  Before timing, the two forwards are compared at the timed size (norm-wise).  Prints ONE JSON line.
    python tools/bench_recurrent.py [--reps 10] [--warmup 2] [--rounds 2] [--graphs 64] [--T 12] [--out 64]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graphneuralnetworks.jl_amd"))

import gnnmp  # noqa: E402

CIN = 2


def road(n, deg=8, seed=0):
    """ring + chords to the next few nodes, bidirected, 1-based, with one weight per undirected pair (tools/bench_tgcn.py's shape)"""
    rng = np.random.default_rng(seed)
    i = np.repeat(np.arange(n), deg // 2)
    j = (i + rng.integers(1, 12, i.size)) % n
    e = np.unique(np.stack([np.minimum(i, j), np.maximum(i, j)], 1), axis=0)
    w = rng.uniform(0.05, 0.2, len(e)).astype(np.float32)          # weighted degrees near 1: the diffusion neither dies nor blows up
    s, t = np.concatenate([e[:, 0], e[:, 1]]), np.concatenate([e[:, 1], e[:, 0]])
    return s.astype(np.int64) + 1, t.astype(np.int64) + 1, np.concatenate([w, w])


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


def composed(kind, cell, g, x, cheb, dconv):
    """the reference's cell, scanned: `cheb(l, g, v)` / `dconv(l, g, v)` are the convolutions (the plain forwards or the *_ad ones)"""
    N, T, _ = x.shape
    h = torch.zeros((N, cell.out), device=x.device)
    c = torch.zeros_like(h)
    ys = []
    for t in range(T):
        xt = x[:, t].contiguous()
        if kind == "gconv_gru":
            r = torch.sigmoid(cheb(cell.conv_x_r, g, xt) + cheb(cell.conv_h_r, g, h))
            z = torch.sigmoid(cheb(cell.conv_x_z, g, xt) + cheb(cell.conv_h_z, g, h))
            ht = torch.tanh(cheb(cell.conv_x_h, g, xt) + cheb(cell.conv_h_h, g, (r * h).contiguous()))
            h = (1 - z) * ht + z * h
        elif kind == "gconv_lstm":
            i = torch.sigmoid(cheb(cell.conv_x_i, g, xt) + cheb(cell.conv_h_i, g, h) + cell.w_i * c + cell.b_i)
            f = torch.sigmoid(cheb(cell.conv_x_f, g, xt) + cheb(cell.conv_h_f, g, h) + cell.w_f * c + cell.b_f)
            c = f * c + i * torch.tanh(cheb(cell.conv_x_c, g, xt) + cheb(cell.conv_h_c, g, h) + cell.w_c * c + cell.b_c)
            o = torch.sigmoid(cheb(cell.conv_x_o, g, xt) + cheb(cell.conv_h_o, g, h) + cell.w_o * c + cell.b_o)
            h = o * torch.tanh(c)
        else:
            xh = torch.cat([xt, h], 1)
            z = torch.sigmoid(dconv(cell.dconv_u, g, xh))
            r = torch.sigmoid(dconv(cell.dconv_r, g, xh))
            cand = torch.tanh(dconv(cell.dconv_c, g, torch.cat([xt, h * r], 1)))
            h = z * h + (1 - z) * cand
        ys.append(h)
    return torch.stack(ys, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--graphs", type=int, default=64)
    ap.add_argument("--T", type=int, default=12)
    ap.add_argument("--out", type=int, default=64)
    a = ap.parse_args()
    gs = []
    for k in range(a.graphs):
        s, t, w = road(207, seed=10 + k)
        gs.append(gnnmp.GNNGraph(torch.from_numpy(s).cuda(), torch.from_numpy(t).cuda(), torch.from_numpy(w).cuda(), num_nodes=207))
    g = gnnmp.batch(gs)
    N = g.num_nodes
    gen = torch.Generator().manual_seed(0)
    x = (torch.rand((N, a.T, CIN), generator=gen) - 0.5).cuda()
    dy = (torch.rand((N, a.T, a.out), generator=gen) - 0.5).cuda()
    res = {"bench": "recurrent", "device": torch.cuda.get_device_name(0), "N": N, "E": g.num_edges, "T": a.T, "in": CIN, "out": a.out,
           "cheb_K": 3, "diffusion_k": 2, "ms": {}, "forward_rel_diff": {}}
    entries = []
    for kind, make, ad in (("gconv_gru", gnnmp.GConvGRU, gnnmp.gconv_gru_ad), ("gconv_lstm", gnnmp.GConvLSTM, gnnmp.gconv_lstm_ad),
                           ("dcgru", gnnmp.DCGRU, gnnmp.dcgru_ad)):
        layer = make((CIN, a.out), 2 if kind == "dcgru" else 3, seed=3)
        cell = layer.cell
        params = [p.requires_grad_() for p in cell.parameters() if p is not None]

        def fwd(layer=layer):
            with torch.no_grad():
                return layer(g, x)

        def fwd_c(kind=kind, cell=cell):
            with torch.no_grad():
                return composed(kind, cell, g, x, gnnmp.cheb_conv, gnnmp.d_conv)

        def train(layer=layer, ad=ad, params=params):
            xd = x.detach().requires_grad_()
            return torch.autograd.grad(ad(layer, g, xd), [xd] + params, dy)

        def train_c(kind=kind, cell=cell, params=params):
            xd = x.detach().requires_grad_()
            return torch.autograd.grad(composed(kind, cell, g, xd, gnnmp.cheb_conv_ad, gnnmp.d_conv_ad), [xd] + params, dy)
        u, v = fwd(), fwd_c()
        res["forward_rel_diff"][kind] = float((u - v).norm() / v.norm())
        entries += [(kind + "_forward", fwd), (kind + "_forward_composed", fwd_c), (kind + "_train", train), (kind + "_train_composed", train_c)]
    for name, _ in entries:
        res["ms"][name] = []
    for _ in range(a.rounds):
        for name, fn in entries:
            res["ms"][name].append(round(timed(fn, a.reps, a.warmup), 4))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
