#!/usr/bin/env python
"""Times GATConv's pullback with edge features (gnnmp_gat_conv_edge_grad_f32) next to the e-less two-pass pullback
(gnnmp_gat_conv_grad_f32) on the same plans and width: the products shape of tools/backward_bench.py, H = 8, C = 16, no self loops
(edge features forbid them).  The difference is the edge term: one 4 H-byte gather of es_k per edge in each pass and one 4 H-byte store
of des_k per edge in the source pass.  --small: a 100 k-node graph (a quick look, not a figure to quote)."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "graphneuralnetworks.jl_amd")):
    sys.path.insert(0, p)
import torch, gnnmp
from gnnmp import synth, backward as bw, _lib as L

def t(fn, it=10):
    fn(); torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(it)]
    for a, b in ev:
        a.record(); fn(); b.record()
    torch.cuda.synchronize()
    ts = sorted(a.elapsed_time(b) for a, b in ev)
    return ts[len(ts) // 2]

small = "--small" in sys.argv
N, E = (100_000, 2_000_000) if small else (synth.PRODUCTS["N"], synth.PRODUCTS["E"])
s, tt = synth.products_like(N=N, E=E)
g = gnnmp.GNNGraph(torch.from_numpy(s).cuda(), torch.from_numpy(tt).cuda(), num_nodes=N, _validated=True)
lib = L.load(); H, C = 8, 16; D = H * C
plan, plan_t = g.plan(False), bw.plan_transposed(g, False)
f = dict(device="cuda")
Wx = torch.randn((N, D), **f) * 0.3; a_hc = torch.randn((H, 2 * C), **f) * 0.3; es = torch.randn((E, H), **f) * 0.3
dy = torch.randn((N, D), **f)
out = torch.empty((N, D), **f); stats = torch.empty((N, H, 2), **f); stats_e = torch.empty((N, H, 2), **f)
line = torch.empty((N, H, 4), **f); dsd = torch.empty((N, H), **f); dss = torch.empty((N, H), **f)
dWx = torch.empty((N, D), **f); da = torch.empty((H, 2 * C), **f); des = torch.empty((E, H), **f)
tf = t(lambda: L.check(lib.gnnmp_gat_conv_stats_f32(plan.handle, L.ptr(Wx), None, L.ptr(a_hc), 0.2, None, 0, L.ptr(out), L.ptr(stats), H, C, L.stream_ptr())))
tfe = t(lambda: L.check(lib.gnnmp_gat_conv_edge_stats_f32(plan.handle, L.ptr(Wx), None, L.ptr(a_hc), L.ptr(es), 0.2, None, 0, L.ptr(out), L.ptr(stats_e), H, C, L.stream_ptr())))
tb = t(lambda: L.check(lib.gnnmp_gat_conv_grad_f32(plan.handle, plan_t.handle, L.ptr(Wx), None, L.ptr(a_hc), 0.2, L.ptr(stats), L.ptr(dy), L.ptr(line), L.ptr(dsd), L.ptr(dss), L.ptr(dWx), None, L.ptr(da), H, C, L.stream_ptr())))
job = L.GatEdgeGradJob(L.ptr(Wx), None, L.ptr(a_hc), L.ptr(es), L.ptr(stats_e), L.ptr(dy), L.ptr(line), L.ptr(dsd), L.ptr(dss), L.ptr(dWx), None, L.ptr(da), L.ptr(des), 0.2)
tbe = t(lambda: L.check(lib.gnnmp_gat_conv_edge_grad_f32(plan.handle, plan_t.handle, job, H, C, L.stream_ptr())))
extra = E * 4 * H * 3      # es_k gathered in both passes, des_k stored once
print(f"GAT pullback, N={N} E={E} H={H} C={C}, no self loops: forward+stats {tf:.3f} ms, with es {tfe:.3f} ms | "
      f"gnnmp_gat_conv_grad_f32 {tb:.3f} ms | gnnmp_gat_conv_edge_grad_f32 {tbe:.3f} ms (+{tbe - tb:.3f} ms for {extra / 1e6:.0f} MB of edge-term traffic)")
