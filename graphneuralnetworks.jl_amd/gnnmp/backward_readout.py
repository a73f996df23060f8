"""The attention readouts, differentiable: Set2Set (GNNlib/src/layers/pool.jl:29-43) and GlobalAttentionPool (pool.jl:7-12) trained on
libgnnmp — forward and pullback on the fused segment kernels of csrc/readout.hip (include/gnnmp.h states the arithmetic).

Both readouts are a per-graph softmax-weighted sum over the graph's contiguous rows.  One gnnmp_segment_attn_pool_f32 call gives r [G][D]
and the softmax's (max, denominator) per graph; one gnnmp_segment_attn_pool_grad_f32 call is the whole pullback, the weights recomputed
from those two numbers.  Nothing of N rows is written by a forward, and nothing of N rows is kept for the backward but x itself.

    set2set_ad    per iteration   gx = [q | r] Wi', gh = h Wh'                          gnnmp_dense_f32 (Wi by column blocks, no vcat)
                                  (h, c) = LSTM pointwise                               gnnmp_lstm_pointwise_f32
                                  q = h,  r = Σ_n softmax_n(q . x_n) x_n                gnnmp_segment_attn_pool_f32 (query mode)
                  kept per iteration: gx, gh, c, q, r, stats — all [G]-sized
                  backward, reverse time, ONE autograd.Function:
                                  (dq, dx += ...) from dr                               gnnmp_segment_attn_pool_grad_f32, base = dx
                                  (da, dc) from dh = dq + (what the next step sent)     gnnmp_lstm_pointwise_grad_f32
                                  d[q | r] = da Wi, dh = da Wh                          dense_grad_x
                  dWi, dWh, db from the T·G stacked rows of da                          gnnmp_dense_grad_w_f32, one call per weight
    global_attention_pool_ad      gate = fgate(x), feats = ffeat(x) through dense_ad; r = Σ_n softmax_n(gate) ⊙ feats in gate mode

torch allocates, slices, stacks and chains; every arithmetic step is a libgnnmp call.  `gnnmp.set2set_pool` and
`gnnmp.global_attention_pool` are unchanged; the fused forwards sum in another order and owe them the 1e-5 bar, not equal bits.
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib as L
from .backward import _act_code, dense_ad, dense_grad_w, dense_grad_x
from .graph import GNNGraph, check_num_nodes, graph_indicator
from .layers import Dense, dense
from .layers_more import _add


def _p(t):
    """the device pointer, NULL for None and for an empty tensor"""
    return None if t is None or t.numel() == 0 else L.ptr(t)


def node_ptr(g: GNNGraph):
    """the int64 [G+1] row offsets of the member graphs: a constant of the batch, cached like its plans (gnnmp/utils.py shares it)"""
    sp = g._cache.get("node_ptr")
    if sp is None:
        gi = graph_indicator(g)
        sp = torch.empty(g.num_graphs + 1, dtype=torch.int64, device=gi.device)
        L.check(L.load().gnnmp_segment_bounds(L.ptr(gi), gi.element_size(), g.index_base, g.num_nodes, g.num_graphs, L.ptr(sp),
                                              L.stream_ptr()))
        g._cache["node_ptr"] = sp
    return sp


def segment_attn_pool(x, sp, q=None, gate=None):
    """(r [G][D], stats [G][max(Dg,1)][2]) of gnnmp_segment_attn_pool_f32: q [G][D] (query mode) or gate [N][1 | D] (gate mode)"""
    N, D = x.shape
    G = sp.numel() - 1
    Dg = 0 if gate is None else gate.shape[1]
    r = torch.empty((G, D), dtype=torch.float32, device=x.device)
    stats = torch.empty((G, max(Dg, 1), 2), dtype=torch.float32, device=x.device)
    if N == 0 or G == 0:      # nothing is launched: every segment is empty
        return r.zero_(), stats.zero_()
    job = L.SegmentAttnJob(_p(x), _p(sp), _p(q), _p(gate), _p(r), _p(stats))
    L.check(L.load().gnnmp_segment_attn_pool_f32(ctypes.byref(job), N, G, D, Dg, L.stream_ptr()))
    return r, stats


def segment_attn_pool_grad(dr, x, sp, r, stats, q=None, gate=None, base=None, want_dq=True, want_dx=True, want_dgate=True):
    """(dq [G][D] | None, dx [N][D] | None, dgate [N][Dg] | None) of gnnmp_segment_attn_pool_grad_f32.  `base` [N][D] is added into dx
    and BECOMES dx (the kernel reads and writes it in place)."""
    N, D = x.shape
    G = sp.numel() - 1
    Dg = 0 if gate is None else gate.shape[1]
    dq = torch.empty((G, D), dtype=torch.float32, device=x.device) if (gate is None and want_dq) else None
    dx = (base if base is not None else torch.empty_like(x)) if want_dx else None
    dgate = torch.empty_like(gate) if (gate is not None and want_dgate) else None
    if dq is None and dx is None and dgate is None:
        return None, None, None
    if N == 0 or G == 0:
        return (None if dq is None else dq.zero_()), dx, dgate
    job = L.SegmentAttnGradJob(_p(dr), _p(x), _p(sp), _p(q), _p(gate), _p(r), _p(stats), _p(base) if want_dx else None, _p(dq), _p(dx),
                               _p(dgate))
    L.check(L.load().gnnmp_segment_attn_pool_grad_f32(ctypes.byref(job), N, G, D, Dg, L.stream_ptr()))
    return dq, dx, dgate


def lstm_pointwise_grad(gx, gh, b, c, dh, dcn=None):
    """(da [G][4D], dc [G][D]) of gnnmp_lstm_pointwise_grad_f32"""
    G, D = c.shape
    da = torch.empty((G, 4 * D), dtype=torch.float32, device=c.device)
    dc = torch.empty_like(c)
    if G > 0:
        job = L.LstmGradJob(_p(gx), _p(gh), _p(b), _p(c), _p(dh), _p(dcn), _p(da), _p(dc))
        L.check(L.load().gnnmp_lstm_pointwise_grad_f32(ctypes.byref(job), G, D, L.stream_ptr()))
    return da, dc


class _Set2SetFn(torch.autograd.Function):
    """(x, Wi, Wh, b) -> vcat(q_T, r_T) [G][2 n_in]"""

    @staticmethod
    def forward(ctx, x, Wi, Wh, b, g, num_iters):
        N, n = x.shape
        G = g.num_graphs
        sp = node_ptr(g)
        lib = L.load()
        z = lambda: torch.zeros((G, n), dtype=torch.float32, device=x.device)
        q, r, c = z(), z(), z()
        steps = []
        for _ in range(num_iters):
            gx = dense(q, Wi[:, :n], None, None, x2=r, W2=Wi[:, n:])      # Wi * vcat(q, r) without the vcat
            gh = dense(q, Wh)                                              # h = q
            hn, cn = torch.empty_like(q), torch.empty_like(c)
            if G > 0:
                L.check(lib.gnnmp_lstm_pointwise_f32(L.ptr(gx), L.ptr(gh), L.ptr(b), L.ptr(c), L.ptr(hn), L.ptr(cn), G, n, L.stream_ptr()))
            rn, stats = segment_attn_pool(x, sp, q=hn)
            steps.append((gx, gh, c, q, r, hn, rn, stats))       # c, q, r: what ENTERED the step; hn, rn: what it made
            q, r, c = hn, rn, cn
        ctx.save_for_backward(x, Wi, Wh, b)
        ctx.steps, ctx.sp = steps, sp
        return torch.cat([q, r], dim=1)                           # vcat(q, r): memory plumbing

    @staticmethod
    def backward(ctx, dout):
        x, Wi, Wh, b = ctx.saved_tensors
        need_x, need_wi, need_wh, need_b = ctx.needs_input_grad[:4]
        need_w = need_wi or need_wh or need_b
        n = x.shape[1]
        T = len(ctx.steps)
        if T == 0 or not (need_x or need_w):
            return (torch.zeros_like(x) if need_x else None), None, None, None, None, None
        dout = dout.contiguous()
        dh_out, dr = dout[:, :n].contiguous(), dout[:, n:].contiguous()      # what reaches q_t = h_t from later steps, and r_t
        dcn, dx, das = None, None, []
        for t in range(T - 1, -1, -1):
            gx, gh, c_in, q_in, r_in, q, r, stats = ctx.steps[t]
            first = t == 0      # its dq reaches the weights only: q_0 = r_0 = h_0 = c_0 = 0 carry nothing further back
            dq, dx, _ = segment_attn_pool_grad(dr, x, ctx.sp, r, stats, q=q, base=dx, want_dq=need_w or not first, want_dx=need_x)
            if first and not need_w:
                break
            da, dcn = lstm_pointwise_grad(gx, gh, b, c_in, _add(dh_out, dq), dcn)
            das.append(da)
            if not first:
                dqs = dense_grad_x(da, Wi)                         # d vcat(q, r) [G][2n]
                dh_out = _add(dqs[:, :n].contiguous(), dense_grad_x(da, Wh))
                dr = dqs[:, n:].contiguous()
        dWi = dWh = db = None
        if need_w:
            DA = torch.cat(das[::-1], dim=0)                       # [T·G][4n], time-major
            if need_wi or need_b:
                qs = torch.cat([torch.cat([s[3], s[4]], dim=1) for s in ctx.steps], dim=0)
                dWi, db = dense_grad_w(DA, qs, need_w=need_wi, need_b=need_b)
            if need_wh:
                dWh = dense_grad_w(DA, torch.cat([s[3] for s in ctx.steps], dim=0), need_b=False)[0]
        if need_x and dx is None:
            dx = torch.zeros_like(x)
        return dx, dWi, dWh, db, None, None


def set2set_ad(l, g: GNNGraph, x):
    """differentiable Set2Set forward -> [num_graphs][2 n_in]: gradients w.r.t. x, l.Wi, l.Wh and l.b.  One fused segment kernel per
    iteration in place of broadcast_nodes, rowdot, softmax_nodes, mul_rows and reduce_nodes; the outputs agree with gnnmp.set2set_pool to
    the 1e-5 bar, not bit for bit."""
    if not isinstance(x, torch.Tensor) or x.dim() != 2:
        raise ValueError("set2set_ad: x must be an [N][n_in] matrix")
    if x.dtype != torch.float32:
        raise ValueError(f"set2set_ad: Float32 only, not {x.dtype} (DESIGN.md §7)")
    n = x.shape[1]
    if tuple(l.Wi.shape) != (4 * n, 2 * n) or tuple(l.Wh.shape) != (4 * n, n):
        raise ValueError(f"set2set_ad: x has {n} features, the LSTM cell was built for {l.Wh.shape[1]}")
    if not 1 <= n <= L.READOUT_MAX_D:
        raise ValueError(f"set2set_ad: n_in = {n} outside 1 .. {L.READOUT_MAX_D}")
    check_num_nodes(g, x)
    return _Set2SetFn.apply(x.contiguous(), l.Wi, l.Wh, l.b, g, l.num_iters)


class _GateAttnPoolFn(torch.autograd.Function):
    """(feats [N][D], gate [N][1 | D]) -> r [G][D]"""

    @staticmethod
    def forward(ctx, feats, gate, g):
        sp = node_ptr(g)
        r, stats = segment_attn_pool(feats, sp, gate=gate)
        ctx.save_for_backward(feats, gate, r, stats)
        ctx.sp = sp
        return r

    @staticmethod
    def backward(ctx, dr):
        feats, gate, r, stats = ctx.saved_tensors
        need_f, need_g = ctx.needs_input_grad[:2]
        _, dfeats, dgate = segment_attn_pool_grad(dr.contiguous(), feats, ctx.sp, r, stats, gate=gate, want_dx=need_f, want_dgate=need_g)
        return dfeats, dgate, None


def _dense_chain(name, chain):
    """fgate / ffeat as a list of gnnmp.Dense whose σ dense_ad carries; ValueError otherwise"""
    layers = list(chain) if isinstance(chain, (list, tuple)) else [chain]
    if not layers:
        raise ValueError(f"global_attention_pool_ad: {name} is empty")
    for k, layer in enumerate(layers):
        if not isinstance(layer, Dense):
            raise ValueError(f"global_attention_pool_ad: layer {k} of {name} is a {type(layer).__name__}; the adjoint covers gnnmp.Dense "
                             "layers only")
        try:
            _act_code(layer.sigma)
        except ValueError:
            raise ValueError(f"global_attention_pool_ad: σ = {layer.sigma!r} in {name}; dense_ad carries identity and relu") from None
    return layers


def global_attention_pool_ad(l, g: GNNGraph, x):
    """differentiable GlobalAttentionPool forward -> [num_graphs][D']: gradients w.r.t. x and every weight and bias of l.fgate and
    l.ffeat, each a gnnmp.Dense or a list of them (σ identity or relu; ffeat = None is the identity).  The gate has one channel or D'."""
    fgate = _dense_chain("fgate", l.fgate)
    ffeat = [] if l.ffeat is None else _dense_chain("ffeat", l.ffeat)
    if not isinstance(x, torch.Tensor) or x.dim() != 2:
        raise ValueError("global_attention_pool_ad: x must be an [N][D] matrix")
    if x.dtype != torch.float32:
        raise ValueError(f"global_attention_pool_ad: Float32 only, not {x.dtype} (DESIGN.md §7)")
    Dg = fgate[-1].weight.shape[0]
    Df = ffeat[-1].weight.shape[0] if ffeat else x.shape[1]
    if Dg not in (1, Df):
        raise ValueError(f"global_attention_pool_ad: the gate has {Dg} channels; it must have one or as many as the features ({Df})")
    if not 1 <= Df <= L.READOUT_MAX_D:
        raise ValueError(f"global_attention_pool_ad: {Df} features outside 1 .. {L.READOUT_MAX_D}")
    check_num_nodes(g, x)
    x = x.contiguous()
    gate, feats = x, x
    for layer in fgate:
        gate = dense_ad(layer, gate)
    for layer in ffeat:
        feats = dense_ad(layer, feats)
    return _GateAttnPoolFn.apply(feats.contiguous(), gate.contiguous(), g)
