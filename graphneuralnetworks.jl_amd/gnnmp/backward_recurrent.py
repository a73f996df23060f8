"""GConvGRU, GConvLSTM and DCGRU, differentiable (gnnmp/layers_temporal.py; GraphNeuralNetworks/src/layers/temporalconv.jl:237-254, 416-437,
564-575): one autograd.Function a layer, forward and pullback on the panel hop (gnnmp_poly_hop_ld_f32) and the fused gate kernels
(csrc/recurrent.hip; include/gnnmp.h states the arithmetic).

The forward is recurrent_forward call for call — layer(g, x) and *_ad(layer, g, x) have equal bits.  Reverse time, per step:
    the gate pullback                      ΔP[t], and the pre-activation gradients contiguous for the next product
    dense_grad_x with the stacked weight   the panel's cotangent [N][B out]: its blocks are the Clenshaw addends G_k
    the Clenshaw recurrence                of backward_poly.py, over the transposed plan, on the panel hop, reading those blocks in place;
                                           block 0 (DConv: blocks 0 + 1) is then the cotangent of the state
    GRU cells                              then phase 0's pullback and the second basis likewise
as many launches as the forward's step (DCGRU with k >= 3: k - 2 more per basis, the Σ_{j >= 2} C_j of d_conv_ad).  After the loop, over
all N T rows at once: the stacked weight gradients (dense_grad_w: the x side against the stacked x basis, the state side against the
panels of all steps, kept time-major so that each step's is contiguous — only when a weight gradient is asked for), the column sums for
the biases and the peepholes, and the x side's pullback at width T in.  Graph weights and λmax are constants of the graph, as in
cheb_conv_ad.  No atomics anywhere; what needs_input_grad rules out is not computed.
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib as L
from .backward import dense_grad_w, dense_grad_x
from .graph import GNNGraph
from .layers_more import _add
from .layers_temporal import (DCGRUCell, GConvGRUCell, GConvLSTMCell, _at, _blk, _check_recurrent_input, recurrent_forward)


def _colsum(m):
    return dense_grad_w(m, m, need_w=False)[1]


def _state_cot(G, part, rep, D):
    """part + Σ_{j < rep} block j of the panel cotangent G (either may be None), contiguous [N][D]"""
    tot = part
    if G is not None:
        for j in range(rep):
            b = _blk(G, j, D).contiguous()
            tot = b if tot is None else _add(tot, b)
    return tot


def _x_pullback(basis, dP2, Wx, N, T, cin):
    """Δx [N][T][in] from ΔP [N T][G out]: one dense, one de-interleaving copy, the basis' pullback at width T in"""
    W = T * cin
    dXb = dense_grad_x(dP2, Wx)                                                     # [N T][B in]
    Gx = dXb.view(N, T, basis.B, cin).permute(0, 2, 1, 3).contiguous().view(N, basis.B * W)
    basis.pullback(Gx, W)
    return _state_cot(Gx, None, basis.rep, W).view(N, T, cin)


def _reduce_state(d, stride):
    """the cotangent of a state given as one vector for every node: its column sum"""
    return d if stride else _colsum(d)


class _RecurrentFn(torch.autograd.Function):
    """arguments: x, h0, c0 (None for the GRU cells), cell, g, then cell.parameters()"""

    @staticmethod
    def forward(ctx, x, h0, c0, cell, g, *params):
        lstm = isinstance(cell, GConvLSTMCell)
        need_w = any(ctx.needs_input_grad[5:])
        y, _, _, sv = recurrent_forward(cell, g, x, (h0, c0) if lstm else h0, keep=need_w)
        if not need_w:
            sv["pan1"] = sv["pan2"] = sv["Xb"] = None
        ctx.cell, ctx.g, ctx.sv, ctx.need_w = cell, g, sv, need_w
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        cell, sv = ctx.cell, ctx.sv
        dy = dy.contiguous()
        if isinstance(cell, GConvLSTMCell):
            return _lstm_backward(ctx, cell, sv, y, dy)
        return _gru_backward(ctx, cell, sv, y, dy)


def _gru_backward(ctx, cell, sv, y, dy):
    N, T, D = y.shape
    basis, Wx, (Wrz, Wc), gates = sv["basis"], sv["Wx"], sv["Wh"], sv["gates"]
    rep, BD = basis.rep, basis.B * D
    h0, ldh0 = sv["h0"], sv["ldh0"]
    need_x, need_h0, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1] and h0 is not None, ctx.need_w
    lib = L.load()
    f32 = dict(dtype=torch.float32, device=dy.device)
    dP = torch.empty((N, T, 3 * D), **f32)
    nk = T if need_w else 1
    dArz, dAc = torch.empty((nk, N, 2 * D), **f32), torch.empty((nk, N, D), **f32)      # time-major like the panels
    carry = G1 = None
    for t in range(T - 1, -1, -1):
        hp, ldh = (_at(y, (t - 1) * D), T * D) if t > 0 else (L.ptr(h0), ldh0)
        dac, darz = dAc[t if need_w else 0], dArz[t if need_w else 0]
        part = torch.empty((N, D), **f32)
        job = L.GruCellGradJob(L.ptr(dy), L.ptr(carry), L.ptr(G1), BD, L.ptr(gates), hp, ldh, None, BD, rep, L.ptr(dP), L.ptr(dac),
                               L.ptr(darz), L.ptr(part))
        if N:
            L.check(lib.gnnmp_gru_cell_grad_f32(1, ctypes.byref(job), N, T, t, D, L.stream_ptr()))
        G2 = dense_grad_x(dac, Wc)                          # the cotangent of the panel of r .* h
        basis.pullback(G2, D)
        job = L.GruCellGradJob(None, None, None, BD, L.ptr(gates), hp, ldh, L.ptr(G2), BD, rep, L.ptr(dP), None, L.ptr(darz), L.ptr(part))
        if N:
            L.check(lib.gnnmp_gru_cell_grad_f32(0, ctypes.byref(job), N, T, t, D, L.stream_ptr()))
        carry, G1 = part, None
        if t > 0 or need_h0:
            G1 = dense_grad_x(darz, Wrz)                    # the cotangent of the panel of h
            basis.pullback(G1, D)
    dh0 = _reduce_state(_state_cot(G1, carry, rep, D), ldh0) if need_h0 else None
    dP2 = dP.view(N * T, 3 * D)
    dx = _x_pullback(basis, dP2, Wx, N, T, cell.in_) if need_x else None
    grads = [None] * len(cell.parameters())
    if need_w:
        dWx, db = dense_grad_w(dP2, sv["Xb"], need_b=sv["has_bias"])
        dWrz = dense_grad_w(dArz.view(T * N, 2 * D), sv["pan1"].view(T * N, BD), need_b=False)[0]
        dWc = dense_grad_w(dAc.view(T * N, D), sv["pan2"].view(T * N, BD), need_b=False)[0]
        dWh = torch.cat([dWrz, dWc])
        grads = _unstack(cell, basis, dWx, dWh, db)
    return (dx, dh0, None, None, None, *[gr if need else None for gr, need in zip(grads, ctx.needs_input_grad[5:])])


def _lstm_backward(ctx, cell, sv, y, dy):
    N, T, D = y.shape
    basis, Wx, (Wh,), gates, w, cs = sv["basis"], sv["Wx"], sv["Wh"], sv["gates"], sv["w"], sv["cs"]
    BD = basis.B * D
    h0, c0, ldc0 = sv["h0"], sv["c0"], sv["ldc0"]
    need_x, need_w = ctx.needs_input_grad[0], ctx.need_w
    need_h0, need_c0 = ctx.needs_input_grad[1] and h0 is not None, ctx.needs_input_grad[2] and c0 is not None
    lib = L.load()
    f32 = dict(dtype=torch.float32, device=dy.device)
    dP = torch.empty((N, T, 4 * D), **f32)
    peep = torch.empty((N, T, 4 * D), **f32) if need_w else None
    dA = torch.empty((T if need_w else 1, N, 4 * D), **f32)
    Gp = dc = None
    for t in range(T - 1, -1, -1):
        cp, ldc = (_at(cs, (t - 1) * D), T * D) if t > 0 else (L.ptr(c0), ldc0)
        da = dA[t if need_w else 0]
        dcn = torch.empty((N, D), **f32)
        job = L.LstmCellGradJob(L.ptr(dy), L.ptr(Gp), BD, L.ptr(dc), L.ptr(gates), L.ptr(w), cp, ldc, L.ptr(cs), L.ptr(dP), L.ptr(da),
                                L.ptr(dcn), L.ptr(peep))
        if N:
            L.check(lib.gnnmp_lstm_cell_grad_f32(ctypes.byref(job), N, T, t, D, L.stream_ptr()))
        dc, Gp = dcn, None
        if t > 0 or need_h0:
            Gp = dense_grad_x(da, Wh)                       # block 0 after the recurrence: the cotangent of h_{t-1}
            basis.pullback(Gp, D)
    dh0 = _reduce_state(_blk(Gp, 0, D).contiguous(), sv["ldh0"]) if need_h0 else None
    dc0 = _reduce_state(dc, ldc0) if need_c0 else None
    dP2 = dP.view(N * T, 4 * D)
    dx = _x_pullback(basis, dP2, Wx, N, T, cell.in_) if need_x else None
    grads = [None] * len(cell.parameters())
    if need_w:
        dWx, db = dense_grad_w(dP2, sv["Xb"], need_b=sv["has_bias"])
        dWh = dense_grad_w(dA.view(T * N, 4 * D), sv["pan1"].view(T * N, BD), need_b=False)[0]
        grads = _unstack(cell, basis, dWx, dWh, db, _colsum(peep.view(N * T, 4 * D)))
    return (dx, dh0, dc0, None, None, *[gr if need else None for gr, need in zip(grads, ctx.needs_input_grad[5:])])


def _unstack(cell, basis, dWx, dWh, db, dpeep=None):
    """the gradients of cell.parameters(), in its order, from those of the stacks: slices and copies; a DConv slice that the stack repeats
    (slice 1, read twice) gets the SUM of its blocks' gradients"""
    D, cin = cell.out, cell.in_
    sl = basis.block_slices()
    per_gate = {}
    for q, n in enumerate(cell.gates):
        gx, gh = dWx[q * D:(q + 1) * D], dWh[q * D:(q + 1) * D]
        gb = None if db is None else db[q * D:(q + 1) * D]
        if isinstance(cell, DCGRUCell):
            acc = {}
            for b, key in enumerate(sl):
                piece = torch.cat([gx[:, b * cin:(b + 1) * cin], gh[:, b * D:(b + 1) * D]], 1)
                acc[key] = piece if key not in acc else _add(acc[key], piece)
            dW = torch.stack([torch.stack([acc[(d, i)] for i in range(cell.k)]) for d in (0, 1)])
            per_gate[n] = [dW, gb]
        else:
            dwx = torch.stack([gx[:, b * cin:(b + 1) * cin] for b in range(len(sl))]).contiguous()
            dwh = torch.stack([gh[:, b * D:(b + 1) * D] for b in range(len(sl))]).contiguous()
            per_gate[n] = [dwx, gb, dwh, gb]
            if dpeep is not None:
                per_gate[n] += [dpeep[q * D:(q + 1) * D], gb]
    order = ("u", "r", "c") if isinstance(cell, DCGRUCell) else cell.gates      # parameters() lists dconv_u first
    return [t for n in order for t in per_gate[n]]


def _apply(name, kind, layer, g, x, state):
    cell = getattr(layer, "cell", layer)
    if not isinstance(cell, kind):
        raise TypeError(f"{name}: expected a {kind.__name__} or its GNNRecurrence, got {type(cell).__name__}")
    _check_recurrent_input(name, cell, g, x)
    if kind is GConvLSTMCell:
        if state is not None and not (isinstance(state, (tuple, list)) and len(state) == 2):
            raise ValueError(f"{name}: the state is a pair (h, c)")
        h0, c0 = state if state is not None else (None, None)
    else:
        h0, c0 = state, None
    for s in (h0, c0):
        if s is not None and s.dtype != torch.float32:
            raise ValueError(f"{name}: the HIP kernels are Float32; the state is {s.dtype}")
    return _RecurrentFn.apply(x.contiguous(), h0, c0, cell, g, *cell.parameters())


def gconv_gru_ad(layer, g: GNNGraph, x, state=None):
    """differentiable GConvGRU / GNNRecurrence(GConvGRUCell) forward: gradients w.r.t. x [N, T, in], the state ([N, out] or [out]) and
    the 12 tensors of GConvGRUCell.parameters()"""
    return _apply("gconv_gru_ad", GConvGRUCell, layer, g, x, state)


def gconv_lstm_ad(layer, g: GNNGraph, x, state=None):
    """differentiable GConvLSTM forward: gradients w.r.t. x, the state pair (h, c) and the 24 tensors of GConvLSTMCell.parameters() (the
    peepholes included)"""
    return _apply("gconv_lstm_ad", GConvLSTMCell, layer, g, x, state)


def dcgru_ad(layer, g: GNNGraph, x, state=None):
    """differentiable DCGRU forward: gradients w.r.t. x, the state and the 6 tensors of DCGRUCell.parameters()"""
    return _apply("dcgru_ad", DCGRUCell, layer, g, x, state)
