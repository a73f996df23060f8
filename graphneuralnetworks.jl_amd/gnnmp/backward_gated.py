"""GatedGraphConv and ResGatedGraphConv, differentiable: the two gated layers trained on libgnnmp.  Both forwards are the existing ones
call for call — under any grad mode they give gnnmp.gated_graph_conv's / gnnmp.res_gated_graph_conv's bits.

gated_graph_conv (GNNlib/src/layers/conv.jl:218-233), per layer i with the state h (x padded with zeros to `dims` columns):

    m = h W_i'                                   gnnmp_dense_f32
    a = propagate(copy_xj, g, aggr; xj = m)      gnnmp_propagate_f32
    gx = a Wi', gh = h Wh'                       gnnmp_dense_f32
    h' = GRU(gx, gh, b, h)                       gnnmp_gru_pointwise_f32

KEPT per layer: h (the state that entered it) and a; for max / min also m (the pullback of the fold compares m with a).  RECOMPUTED in
the backward: gx and gh (two dense calls: the forward's bits) and, inside the kernel, the gates r, z and the candidate h~.  Backward, per
layer in reverse, Δ the cotangent of h':

    (dgx, dgh, dh) = gnnmp_gru_pointwise_grad_f32            dh = Δ z, the direct term
    dWi += dgx' a,  db += colsum(dgx),  dWh += dgh' h        gnnmp_dense_grad_w_f32
    da = dgx Wi,  dh += dgh Wh                               gnnmp_dense_f32 (W read transposed)
    dm = the fold's pullback of da                           propagate_grad_xj: the fused kernel on the transposed plan (+ / mean),
                                                             gnnmp_propagate_maxmin_grad_f32 (max / min)
    dW_i = dm' h,  dh += dm W_i

and Δx is the first m columns of the last dh.

res_gated_graph_conv (conv.jl:287-300): y = σ.(U x_i + Σ_j sigmoid.(A x_i + B x_j) .* V x_j + bias).  The gated message is CGConv's with
act = identity, no edge share and a zero s half on the destination side, so its pullback is gnnmp_cg_conv_grad_f32 on fs_i = [A x | 0],
fs_j = [B x | V x] (csrc/cg_grad.hip) — no new kernel: dz = act_grad(Δ, y), then dfs_i, dfs_j, then the dense adjoints.

torch allocates, slices and chains; every arithmetic step is a libgnnmp call.  What needs_input_grad says is not needed is not computed.
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib as L
from .backward import _act_code, act_grad, dense_grad_w, dense_grad_x, plan_transposed, propagate_grad_xj
from .backward_cg import cg_rows_grad
from .graph import GNNGraph, check_num_nodes
from .layers import bias_act, dense
from .layers_more import _add
from .msgpass import aggr_code


def gru_pointwise_grad(gx, gh, b, h, dout, base=None):
    """(dgx, dgh [N][3D], dh [N][D]) of gnnmp_gru_pointwise_grad_f32; dh = base + Δ z when base [N][D] is given"""
    N, D = h.shape
    dgx, dgh, dh = torch.empty_like(gx), torch.empty_like(gh), torch.empty_like(h)
    if N > 0 and D > 0:
        job = L.GruGradJob(L.ptr(gx), L.ptr(gh), L.ptr(b), L.ptr(h), L.ptr(dout), L.ptr(base), L.ptr(dgx), L.ptr(dgh), L.ptr(dh))
        L.check(L.load().gnnmp_gru_pointwise_grad_f32(ctypes.byref(job), N, D, L.stream_ptr()))
    return dgx, dgh, dh


def _check(name, g, x):
    if isinstance(x, (tuple, list)):
        raise NotImplementedError(f"{name}: a bipartite (xs, xt) input is not covered; pass one feature matrix")
    if x.dtype != torch.float32:
        raise ValueError(f"{name}: the HIP adjoints are Float32; x is {x.dtype}")
    check_num_nodes(g, x)
    if x.dim() != 2:
        raise ValueError(f"{name}: x must be a matrix, not {tuple(x.shape)}")


# ---------------------------------------------------------------------------------------------------------
# GatedGraphConv
# ---------------------------------------------------------------------------------------------------------
class _GatedGraphConvFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, Wi, Wh, b, g, aggr, dims):
        N, m = x.shape
        if m < dims:
            h = torch.zeros((N, dims), dtype=torch.float32, device=x.device)      # vcat(x, zeros): a copy, no arithmetic
            h[:, :m] = x
        else:
            h = x
        plan = g.plan(False)
        lib = L.load()
        code = aggr_code(aggr)
        sel = code in (L.MAX, L.MIN)
        keep = any(ctx.needs_input_grad[:5])
        saved = []
        for i in range(weight.shape[0]):
            mm = dense(h, weight[i])
            agg = torch.empty_like(mm)
            L.check(lib.gnnmp_propagate_f32(plan.handle, L.COPY_XJ, code, L.ptr(mm), None, None, None, L.ptr(agg), dims, L.stream_ptr()))
            gx, gh = dense(agg, Wi), dense(h, Wh)
            out = torch.empty_like(h)
            L.check(lib.gnnmp_gru_pointwise_f32(L.ptr(gx), L.ptr(gh), L.ptr(b), L.ptr(h), L.ptr(out), N, dims, L.stream_ptr()))
            if keep:
                saved += [h, agg] + ([mm] if sel else [])
            h = out
        ctx.save_for_backward(weight, Wi, Wh, *(() if b is None else (b,)), *saved)
        ctx.g, ctx.aggr, ctx.sel, ctx.m, ctx.has_b = g, aggr, sel, m, b is not None
        return h

    @staticmethod
    def backward(ctx, dout):
        weight, Wi, Wh, *rest = ctx.saved_tensors
        b = rest.pop(0) if ctx.has_b else None
        g, sel = ctx.g, ctx.sel
        per = 3 if sel else 2
        nl = weight.shape[0]
        need_x, need_w, need_wi, need_wh = ctx.needs_input_grad[:4]
        need_b = ctx.has_b and ctx.needs_input_grad[4]
        if not (need_x or need_w or need_wi or need_wh or need_b):
            return (None,) * 8
        d = dout.contiguous()
        dWs = [None] * nl
        dWi = dWh = db = None
        acc = lambda a, v: v if a is None else _add(a, v)      # noqa: E731
        for i in range(nl - 1, -1, -1):
            h, agg = rest[per * i], rest[per * i + 1]
            mm = rest[per * i + 2] if sel else None
            last = i == 0 and not need_x      # nothing below the first layer wants dh
            gx, gh = dense(agg, Wi), dense(h, Wh)
            dgx, dgh, dh = gru_pointwise_grad(gx, gh, b, h, d)
            if need_wi or need_b:
                dWi_l, db_l = dense_grad_w(dgx, agg, need_w=need_wi, need_b=need_b)
                if need_wi:
                    dWi = acc(dWi, dWi_l)
                if need_b:
                    db = acc(db, db_l)
            if need_wh:
                dWh = acc(dWh, dense_grad_w(dgh, h, need_b=False)[0])
            if last and not need_w:
                break
            dagg = dense_grad_x(dgx, Wi)
            dmm = propagate_grad_xj(g, ctx.aggr, dagg, xj=mm, y=agg) if sel else propagate_grad_xj(g, ctx.aggr, dagg)
            if need_w:
                dWs[i] = dense_grad_w(dmm, h, need_b=False)[0]
            if last:
                break
            d = _add(_add(dh, dense_grad_x(dgh, Wh)), dense_grad_x(dmm, weight[i]))
        dx = d[:, :ctx.m].contiguous() if need_x else None
        dW = torch.stack(dWs) if need_w else None
        return dx, dW, dWi, dWh, db, None, None, None


def gated_graph_conv_ad(l, g: GNNGraph, x):
    """differentiable GatedGraphConv forward: gradients w.r.t. x (the first m columns of the padded state), l.weight, l.gru_Wi, l.gru_Wh
    and l.gru_b, for +, mean, max and min.  The forward is gnnmp.gated_graph_conv call for call: equal bits.  Kept per layer: the state
    that entered it and the aggregate (max / min: the messages too); gx, gh and the gates are recomputed in the backward."""
    _check("gated_graph_conv_ad", g, x)
    aggr_code(l.aggr)
    if x.shape[1] > l.dims:
        raise ValueError(f"gated_graph_conv_ad: number of input features ({x.shape[1]}) must be less or equal to output features ({l.dims})")
    return _GatedGraphConvFn.apply(x.contiguous(), l.weight, l.gru_Wi, l.gru_Wh, l.gru_b, g, l.aggr, l.dims)


# ---------------------------------------------------------------------------------------------------------
# ResGatedGraphConv
# ---------------------------------------------------------------------------------------------------------
class _ResGatedFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, A, B, U, V, bias, l, g):
        lib = L.load()
        plan = g.plan(False)
        D = A.shape[0]
        BV = l.BV
        Ax = dense(x, A)
        BVx = dense(x, BV)
        m = torch.empty((plan.n_dst, D), dtype=torch.float32, device=x.device)
        L.check(lib.gnnmp_propagate_gated_f32(plan.handle, L.SUM, L.ptr(Ax), L.ptr(BVx), L.ptr(m), D, L.stream_ptr()))
        Ux = dense(x, U)
        L.check(lib.gnnmp_add_f32(L.ptr(Ux), L.ptr(m), L.ptr(Ux), Ux.numel(), L.stream_ptr()))
        y = bias_act(Ux, bias, l.sigma)
        if any(ctx.needs_input_grad[:6]):
            ctx.save_for_backward(x, A, BV, U, Ax, BVx, y)
        ctx.g, ctx.sigma, ctx.has_bias = g, l.sigma, bias is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, A, BV, U, Ax, BVx, y = ctx.saved_tensors
        g = ctx.g
        D = A.shape[0]
        need_x, need_A, need_B, need_U, need_V = ctx.needs_input_grad[:5]
        need_b = ctx.has_bias and ctx.needs_input_grad[5]
        dz = act_grad(dy.contiguous(), y, ctx.sigma)                # cotangent of U x + m + bias: of each summand
        dx = dA = dB = dU = dV = db = None
        if need_U or need_b:
            dU, db = dense_grad_w(dz, x, need_w=need_U, need_b=need_b)
        if need_x or need_A or need_B or need_V:
            fs_i = torch.zeros((x.shape[0], 2 * D), dtype=torch.float32, device=x.device)      # [A x | 0]: a copy, no arithmetic
            fs_i[:, :D] = Ax
            dfs_i, dfs_j, _ = cg_rows_grad(g.plan(False), plan_transposed(g, False), fs_i, BVx, None, dz, L.ACT_IDENTITY, D, want_e=False)
            dAx = dfs_i[:, :D].contiguous()                         # (the s half of dfs_i is the cotangent of the zeros: dropped)
            if need_A:
                dA = dense_grad_w(dAx, x, need_b=False)[0]
            if need_B or need_V:
                dBV = dense_grad_w(dfs_j, x, need_b=False)[0]       # [dB; dV]
                dB = dBV[:D].contiguous() if need_B else None
                dV = dBV[D:].contiguous() if need_V else None
            if need_x:
                dx = _add(_add(dense_grad_x(dz, U), dense_grad_x(dAx, A)), dense_grad_x(dfs_j, BV))
        return dx, dA, dB, dU, dV, db, None, None


def res_gated_graph_conv_ad(l, g: GNNGraph, x):
    """differentiable ResGatedGraphConv forward: gradients w.r.t. x, l.A, l.B, l.U, l.V and l.bias, σ = identity or relu.  The forward is
    gnnmp.res_gated_graph_conv call for call: equal bits."""
    _check("res_gated_graph_conv_ad", g, x)
    try:
        _act_code(l.sigma)
    except ValueError:
        raise ValueError(f"res_gated_graph_conv_ad: σ = {l.sigma!r}; the HIP adjoints of ResGatedGraphConv cover identity and relu") from None
    if x.shape[1] != l.A.shape[1]:
        raise ValueError(f"res_gated_graph_conv_ad: x has {x.shape[1]} features, the layer was built for {l.A.shape[1]}")
    return _ResGatedFn.apply(x.contiguous(), l.A, l.B, l.U, l.V, l.bias, l, g)
