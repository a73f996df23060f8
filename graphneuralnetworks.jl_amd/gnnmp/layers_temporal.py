"""TGCN — the temporal graph convolution of GraphNeuralNetworks/src/layers/temporalconv.jl:

  TGCNCell       temporalconv.jl:809-849   conv_g = GNNChain(GCNConv(in => out, relu; kws...), GCNConv(out => out; kws...)) and
                                           dense_g = Dense(2out => out, σ | tanh) for g in z, r, h; one step
                                             z = dense_z(vcat(conv_z(g, x), h)),  r = dense_r(vcat(conv_r(g, x), h)),
                                             h~ = dense_h(vcat(conv_h(g, x), r .* h)),  h = (1 .- z) .* h .+ z .* h~;  returns (h, h)
  GNNRecurrence  temporalconv.jl:121-135   scans the cell over the time dimension: torch [N, T, in] -> [N, T, out]
  TGCN           temporalconv.jl:884       GNNRecurrence(TGCNCell(args...))

The graph convolutions never see the state, so the spatial work of all T steps and all three gates runs up front in a number of launches
independent of T (phase A: the time steps are columns — [N, T, C] is node-major, so one propagate at width T C serves every step — and the
three chains are stacked side by side, width 3 out).  What is left is node-local, and gnnmp_tgcn_recurrence_f32 runs all T steps in one
launch (csrc/temporal.hip).  For out > 128, or with knob 20 (KNOB_TGCN) < 0, the recurrence runs step by step instead: two gnnmp_dense_f32
products and two pointwise launches per step.

Weights keep the Julia shapes (GCNConv weight (out, in), Dense weight (out, 2out)); every arithmetic step is a libgnnmp call.
"""
from __future__ import annotations

import torch

from . import _lib as L
from .graph import GNNGraph, check_num_nodes
from .layers import Dense, GCNConv, GNNChain, dense, gcn_norm_cache

TGCN_MAX_OUT = 128          # the one-launch recurrence's envelope (csrc/temporal.hip)


class TGCNCell:
    """TGCNCell(in => out; bias=true, add_self_loops=true, use_edge_weight=false) — temporalconv.jl:809-849.  Fields as in the
    reference: in_ (`in` is a Python keyword), out, conv_z / conv_r / conv_h (GNNChain of two GCNConv), dense_z / dense_r / dense_h
    (Dense(2out => out)).  cell(g, x [N, in], h=None) -> (h, h) with h [N, out]; a state h may be [N, out] or [out] (repeated over the
    nodes); None is initialstates, zeros(out)."""

    takes_graph = True

    def __init__(self, ch, bias=True, add_self_loops=True, use_edge_weight=False, device="cuda", seed=None):
        cin, cout = ch
        s = 0 if seed is None else int(seed)
        self.in_, self.out = cin, cout
        kw = dict(bias=bias, add_self_loops=add_self_loops, use_edge_weight=use_edge_weight, device=device)
        for k, (name, sigma) in enumerate((("z", torch.sigmoid), ("r", torch.sigmoid), ("h", torch.tanh))):
            conv = GNNChain(GCNConv((cin, cout), "relu", seed=s + 10 * k + 1, **kw), GCNConv((cout, cout), seed=s + 10 * k + 2, **kw))
            setattr(self, "conv_" + name, conv)
            setattr(self, "dense_" + name, Dense((2 * cout, cout), sigma, device=device, seed=s + 10 * k + 3))

    @property
    def add_self_loops(self):
        return bool(self.conv_z.layers[0].add_self_loops)

    @property
    def use_edge_weight(self):
        return bool(self.conv_z.layers[0].use_edge_weight)

    def parameters(self):
        """the 18 parameter tensors in tgcn_ad's order: per gate z, r, h — conv layer 1 (weight, bias), conv layer 2 (weight, bias),
        dense (weight, bias); a bias is None with bias=false"""
        out = []
        for name in ("z", "r", "h"):
            c1, c2 = getattr(self, "conv_" + name).layers
            d = getattr(self, "dense_" + name)
            out += [c1.weight, c1.bias, c2.weight, c2.bias, d.weight, d.bias]
        return out

    def initialstates(self, device=None):
        return torch.zeros(self.out, dtype=torch.float32, device=device or self.dense_z.weight.device)

    def __call__(self, g, x, h=None):
        y = tgcn_forward(self, g, x.reshape(x.shape[0], 1, x.shape[-1]), h)
        h = y.reshape(y.shape[0], self.out)
        return h, h


class GNNRecurrence:
    """GNNRecurrence(cell) — temporalconv.jl:121-135: layer(g, x [N, T, in], state=None) -> [N, T, out], the cell scanned over the
    time dimension (the reference's dims = 2 of (in, T, N))."""

    takes_graph = True

    def __init__(self, cell):
        self.cell = cell

    def __call__(self, g, x, state=None):
        if isinstance(self.cell, TGCNCell):
            return tgcn_forward(self.cell, g, x, state)
        ys, h = [], state
        for t in range(x.shape[1]):
            h, yt = self.cell(g, x[:, t], h)
            ys.append(yt)
        return torch.stack(ys, 1)


def TGCN(ch, **kw):
    """TGCN(in => out; kws...) = GNNRecurrence(TGCNCell(in => out; kws...)) — temporalconv.jl:884"""
    return GNNRecurrence(TGCNCell(ch, **kw))


# ---------------------------------------------------------------------------------------------------------
# shared pieces of the forward and the pullback (gnnmp/backward_temporal.py)
# ---------------------------------------------------------------------------------------------------------
def _blockdiag(ms):
    """[3out, 3out] with the three [out, out] blocks on the diagonal: the three gates' products as ONE dense launch over N T rows (the
    zeros add exact zeros; the products keep the reference's order — W_g[:, 1:out] is never pre-multiplied into W2_g)"""
    o = ms[0].shape[0]
    out = torch.zeros((3 * o, 3 * o), dtype=torch.float32, device=ms[0].device)
    for k, m in enumerate(ms):
        out[k * o:(k + 1) * o, k * o:(k + 1) * o] = m
    return out


def _cat_bias(bs):
    return None if bs[0] is None else torch.cat(bs).contiguous()


def stacked_params(cell):
    """(W1 [3out, in], b1, W2bd [3out, 3out], b2, Winbd [3out, 3out], bin, U_zr [2out, out], U_h [out, out]); bias None with bias=false"""
    o = cell.out
    c1 = [getattr(cell, "conv_" + n).layers[0] for n in "zrh"]
    c2 = [getattr(cell, "conv_" + n).layers[1] for n in "zrh"]
    d = [getattr(cell, "dense_" + n) for n in "zrh"]
    W1 = torch.cat([c.weight for c in c1]).contiguous()
    W2bd = _blockdiag([c.weight for c in c2])
    Winbd = _blockdiag([l.weight[:, :o] for l in d])
    Uzr = torch.cat([d[0].weight[:, o:], d[1].weight[:, o:]]).contiguous()
    Uh = d[2].weight[:, o:].contiguous()
    return W1, _cat_bias([c.bias for c in c1]), W2bd, _cat_bias([c.bias for c in c2]), Winbd, _cat_bias([l.bias for l in d]), Uzr, Uh


def gcn_propagate(g: GNNGraph, loops: bool, w, h, bias=None, relu=False):
    """GCNConv's normalised aggregation (GNNlib/src/layers/conv.jl:52-70, the norm caches gcn_conv uses) of [N, D] rows, D = T * C; with
    bias / relu the W-first branch's epilogue σ.(x .+ b) (b repeated over the T column blocks by the caller)"""
    plan = g.plan(loops)
    c, c_slot, w_slot = gcn_norm_cache(g, loops, w)
    out = torch.empty((plan.n_dst, h.shape[1]), dtype=torch.float32, device=h.device)
    lib = L.load()
    if bias is not None or relu:
        L.check(lib.gnnmp_propagate_slots_act_f32(plan.handle, L.SUM, L.ptr(h), L.ptr(w_slot), L.ptr(c_slot), L.ptr(c), L.ptr(bias),
                                                  L.ACT_RELU if relu else L.ACT_IDENTITY, L.ptr(out), h.shape[1], L.stream_ptr()))
    else:
        L.check(lib.gnnmp_propagate_slots_f32(plan.handle, L.SUM, L.ptr(h), L.ptr(w_slot), L.ptr(c_slot), L.ptr(c), L.ptr(out), h.shape[1],
                                              L.stream_ptr()))
    return out


def phase_a(cell, g: GNNGraph, x, sp):
    """the three GCN chains and the input halves of the three Dense layers for all T steps: P [N, T, 3out] and what the pullback needs
    (a dict).  Five to six launches whatever T is."""
    W1, b1, W2bd, b2, Winbd, bin_, _, _ = sp
    N, T, cin = x.shape
    o = cell.out
    loops = cell.add_self_loops
    w = g.w if cell.use_edge_weight else None
    xf = x.contiguous()
    sv = {}
    if o >= cin:
        # layer 1, aggregate first (conv.jl:59-71): one propagate of x as [N, T in], shared by the three gates (same normalisation)
        a1 = gcn_propagate(g, loops, w, xf.view(N, T * cin))
        h1 = dense(a1.view(N * T, cin), W1, b1, "relu")
        sv["a1"] = a1
    else:
        # W first (conv.jl:36-40): the stacked product, then one propagate at width T 3out with bias and relu in its epilogue
        u = dense(xf.view(N * T, cin), W1)
        h1 = gcn_propagate(g, loops, w, u.view(N, T * 3 * o), bias=None if b1 is None else b1.repeat(T), relu=True).view(N * T, 3 * o)
    a2 = gcn_propagate(g, loops, w, h1.view(N, T * 3 * o))
    C = dense(a2.view(N * T, 3 * o), W2bd, b2)
    P = dense(C, Winbd, bin_)
    sv.update(x=xf, h1=h1, a2=a2, C=C)
    return P.view(N, T, 3 * o), sv


def state_arg(h, N, out, device):
    """(tensor or None, stride) of a state: None -> zeros; [out] -> one vector for every node (stride 0); [N, out] -> per node"""
    if h is None:
        return None, out
    h = h.to(device=device, dtype=torch.float32).contiguous()
    if h.dim() == 1:
        if h.numel() != out:
            raise ValueError(f"state of size {h.numel()}, expected {out}")
        return h, 0
    if tuple(h.shape) != (N, out):
        raise ValueError(f"state of shape {tuple(h.shape)}, expected ({N}, {out}) or ({out},)")
    return h, out


def use_fused(out):
    return L.knob(L.KNOB_TGCN) >= 0 and out <= TGCN_MAX_OUT


def recurrence(P, Uzr, Uh, h0, h0_stride, need_gates=True):
    """y [N, T, out] (and the saved gates [N, T, 3out]) of the recurrence over P: one launch, or the per-step path"""
    N, T, D3 = P.shape
    o = D3 // 3
    lib = L.load()
    y = torch.empty((N, T, o), dtype=torch.float32, device=P.device)
    fused = use_fused(o)                                     # (one read of the knob per recurrence)
    gates = torch.empty((N, T, 3 * o), dtype=torch.float32, device=P.device) if (need_gates or not fused) else None
    if fused:
        L.check(lib.gnnmp_tgcn_recurrence_f32(L.ptr(P), L.ptr(Uzr), L.ptr(Uh), L.ptr(h0), h0_stride, L.ptr(y), L.ptr(gates), N, T, o,
                                              L.stream_ptr()))
        return y, gates
    h = torch.zeros((N, o), dtype=torch.float32, device=P.device) if h0 is None else h0.expand(N, o).contiguous()
    for t in range(T):
        a = dense(h, Uzr)
        rh = torch.empty((N, o), dtype=torch.float32, device=P.device)
        L.check(lib.gnnmp_tgcn_step_f32(0, L.ptr(P), L.ptr(a), L.ptr(h), o, L.ptr(gates), L.ptr(rh), None, N, T, t, o, L.stream_ptr()))
        a = dense(rh, Uh)
        hn = torch.empty((N, o), dtype=torch.float32, device=P.device)
        L.check(lib.gnnmp_tgcn_step_f32(1, L.ptr(P), L.ptr(a), L.ptr(h), o, L.ptr(gates), L.ptr(hn), L.ptr(y), N, T, t, o,
                                        L.stream_ptr()))
        h = hn
    return y, gates


def tgcn_forward(cell, g: GNNGraph, x, state=None):
    """GNNRecurrence(TGCNCell)(g, x [N, T, in], state) -> [N, T, out] (forward only; tgcn_ad differentiates it)"""
    if x.dim() != 3 or x.shape[2] != cell.in_:
        raise ValueError(f"TGCN input must be [N, T, {cell.in_}], got {tuple(x.shape)}")
    check_num_nodes(g, x)
    N, T, _ = x.shape
    sp = stacked_params(cell)
    P, _ = phase_a(cell, g, x.to(torch.float32), sp)
    h0, stride = state_arg(state, N, cell.out, x.device)
    y, _ = recurrence(P, sp[6], sp[7], h0, stride, need_gates=False)
    return y


