"""Pullback of TGCN (gnnmp/layers_temporal.py; GraphNeuralNetworks/src/layers/temporalconv.jl:809-849, 121-135).

  recurrence   gnnmp_tgcn_recurrence_grad_f32: reverse-time BPTT in one launch -> ΔP [N, T, 3out], Δh0, S = (h_{t-1}, r .* h_{t-1});
               or the per-step path (knob 20 < 0, out > 128): gnnmp_tgcn_step_grad_f32 + two gnnmp_dense_f32 products per step
  weights      ΔW_g[:, 1:out] = ΔP_g' conv_g, ΔU = ΔP' S, Δb_g = colsum(ΔP_g): gnnmp_dense_grad_w_f32 over the N T rows (deterministic slab
               partials, no atomics); the three gates in one call each (the off-diagonal blocks of the [3out, *] results are not used)
  phase A      the two GCN layers' adjoints as in _GCNConvFn: the same propagate on the transposed plan (propagate_grad_xj), act_grad,
               dense_grad_w, dense_grad_x — each at width T C / 3out, so the launch count does not depend on T either
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib as L
from .backward import act_grad, dense_grad_w, dense_grad_x, propagate_grad_xj
from .graph import GNNGraph, check_num_nodes
from .layers_temporal import phase_a, recurrence, stacked_params, state_arg, use_fused


def _at(t, offset_floats):
    return ctypes.c_void_p(t.data_ptr() + 4 * offset_floats)


def recurrence_grad(dy, y, gates, Uzr, Uh, h0, h0_stride):
    """(ΔP [N, T, 3out], S [N, T, 2out], Δh0 [N, out])"""
    N, T, o = y.shape
    lib = L.load()
    f32 = dict(dtype=torch.float32, device=dy.device)
    dP = torch.empty((N, T, 3 * o), **f32)
    S = torch.empty((N, T, 2 * o), **f32)
    if use_fused(o):
        dh0 = torch.empty((N, o), **f32)
        L.check(lib.gnnmp_tgcn_recurrence_grad_f32(L.ptr(dy), L.ptr(y), L.ptr(gates), L.ptr(Uzr), L.ptr(Uh), L.ptr(h0), h0_stride,
                                                   L.ptr(dP), L.ptr(S), L.ptr(dh0), N, T, o, L.stream_ptr()))
        return dP, S, dh0
    h0f = None if h0 is None else h0.expand(N, o).contiguous()
    carry = None
    for t in range(T - 1, -1, -1):
        hp, ldh = (_at(y, (t - 1) * o), T * o) if t > 0 else ((L.ptr(h0f), o) if h0f is not None else (None, o))
        dah = torch.empty((N, o), **f32)
        dzr = torch.empty((N, 2 * o), **f32)
        part = torch.empty((N, o), **f32)
        L.check(lib.gnnmp_tgcn_step_grad_f32(0, L.ptr(dy), L.ptr(carry), L.ptr(gates), hp, ldh, None, L.ptr(dP), L.ptr(dah), L.ptr(dzr),
                                             L.ptr(part), None, N, T, t, o, L.stream_ptr()))
        drh = dense_grad_x(dah, Uh)
        L.check(lib.gnnmp_tgcn_step_grad_f32(1, None, None, L.ptr(gates), hp, ldh, L.ptr(drh), L.ptr(dP), None, L.ptr(dzr), L.ptr(part),
                                             L.ptr(S), N, T, t, o, L.stream_ptr()))
        u = dense_grad_x(dzr, Uzr)
        L.check(lib.gnnmp_add_f32(L.ptr(part), L.ptr(u), L.ptr(part), part.numel(), L.stream_ptr()))
        carry = part
    return dP, S, carry


def _diag_blocks(M, o):
    return [M[k * o:(k + 1) * o, k * o:(k + 1) * o] for k in range(3)]


class _TGCNFn(torch.autograd.Function):
    """GNNRecurrence(TGCNCell) with HIP forward AND backward.  Arguments: x, state, then the 18 parameters of TGCNCell.parameters()."""

    @staticmethod
    def forward(ctx, x, state, cell, g, *params):
        N, T, cin = x.shape
        o = cell.out
        sp = stacked_params(cell)
        P, sv = phase_a(cell, g, x, sp)
        h0, stride = state_arg(state, N, o, x.device)
        y, gates = recurrence(P, sp[6], sp[7], h0, stride)
        ctx.cell, ctx.g, ctx.stride = cell, g, stride
        ctx.has_state = h0 is not None
        ctx.w_first = o < cin
        ctx.sp, ctx.sv = sp, sv
        ctx.save_for_backward(y, gates, h0 if h0 is not None else torch.empty(0, device=x.device))
        return y

    @staticmethod
    def backward(ctx, dy):
        y, gates, h0 = ctx.saved_tensors
        h0 = h0 if ctx.has_state else None
        cell, g, sv = ctx.cell, ctx.g, ctx.sv
        W1, b1, W2bd, b2, Winbd, bin_, Uzr, Uh = ctx.sp
        N, T, o = y.shape
        cin = cell.in_
        NT = N * T
        loops = cell.add_self_loops
        dP, S, dh0 = recurrence_grad(dy.contiguous(), y, gates, Uzr, Uh, h0, ctx.stride)
        dPf = dP.view(NT, 3 * o)
        # the three Dense layers: input halves against conv_g, state halves against S, biases = colsum(ΔP)
        dWin, dbin = dense_grad_w(dPf, sv["C"])
        dU, _ = dense_grad_w(dPf, S.view(NT, 2 * o), need_b=False)
        dWin = _diag_blocks(dWin, o)
        dUg = [dU[0:o, 0:o], dU[o:2 * o, 0:o], dU[2 * o:3 * o, o:2 * o]]
        dWd = [torch.cat([dWin[k], dUg[k]], 1) for k in range(3)]
        dbd = [dbin[k * o:(k + 1) * o] for k in range(3)]
        # layer 2 of the three chains: C = W2bd * A2 + b2
        dC = dense_grad_x(dPf, Winbd)
        dW2, db2 = dense_grad_w(dC, sv["a2"].view(NT, 3 * o), need_b=b2 is not None)
        dA2 = dense_grad_x(dC, W2bd)
        c, _, _ = _norm(g, loops)

        def PT(h):
            return propagate_grad_xj(g, "+", h, scale_src=c, scale_dst=c, add_self_loops=loops)

        dh1 = PT(dA2.view(N, T * 3 * o))
        dz1 = act_grad(dh1.view(NT, 3 * o).contiguous(), sv["h1"], "relu")
        xf = sv["x"]
        dx = None
        if not ctx.w_first:
            dW1, db1 = dense_grad_w(dz1, sv["a1"].view(NT, cin), need_b=b1 is not None)
            if ctx.needs_input_grad[0]:
                dx = PT(dense_grad_x(dz1, W1).view(N, T * cin)).view(N, T, cin)
        else:
            _, db1 = dense_grad_w(dz1, dz1, need_w=False, need_b=b1 is not None)
            du = PT(dz1.view(N, T * 3 * o)).view(NT, 3 * o)
            dW1, _ = dense_grad_w(du, xf.view(NT, cin), need_b=False)
            if ctx.needs_input_grad[0]:
                dx = dense_grad_x(du, W1).view(N, T, cin)
        dstate = None
        if ctx.has_state and ctx.needs_input_grad[1]:
            dstate = dh0 if ctx.stride else dense_grad_w(dh0, dh0, need_w=False)[1]
        grads = []
        dW2 = _diag_blocks(dW2, o)
        for k in range(3):
            grads += [dW1[k * o:(k + 1) * o], None if db1 is None else db1[k * o:(k + 1) * o],
                      dW2[k], None if db2 is None else db2[k * o:(k + 1) * o], dWd[k], dbd[k]]
        return (dx, dstate, None, None, *grads)


def _norm(g, loops):
    from .layers import gcn_norm_cache
    return gcn_norm_cache(g, loops)


def tgcn_ad(layer, g: GNNGraph, x, state=None):
    """differentiable TGCN / GNNRecurrence(TGCNCell) forward: gradients w.r.t. x [N, T, in], the state ([N, out] or [out]) and the 18
    parameter tensors of the cell (TGCNCell.parameters()).  Unweighted graphs only, like gcn_conv_ad: use_edge_weight = true raises."""
    cell = getattr(layer, "cell", layer)
    if cell.use_edge_weight:
        raise NotImplementedError("tgcn_ad: gradients with use_edge_weight = true are not implemented (the forward supports it)")
    if x.dim() != 3 or x.shape[2] != cell.in_:
        raise ValueError(f"TGCN input must be [N, T, {cell.in_}], got {tuple(x.shape)}")
    check_num_nodes(g, x)
    return _TGCNFn.apply(x.contiguous(), state, cell, g, *cell.parameters())
