"""EdgeConv, differentiable: the layer the device-side knn_graph / radius_graph exist for, forward and pullback on libgnnmp.

edge_conv (GNNlib/src/layers/conv.jl:237-246) is propagate(edge_conv_message, g, aggr) with the message nn(vcat(xi, xj .- xi)).  For a
one-layer nn = Dense(2 in => out, σ), W = [W1 | W2]:

    nn(vcat(xi, xj - xi)) = σ(W1 xi + b - W2 xi + W2 xj)

so the contraction is ONE dense call on N rows, P = x [W1; W2]' + [b; 0] ([N][2 out], planar), and the per-edge rest — two additions, σ and
the aggregation — one pass of a row kernel over gathered rows of P (gnnmp_edge_conv_f32, csrc/edge_conv.hip).  The pullback has the
mirrored shape: one pass over the plan and one over the transposed plan give dP (gnnmp_edge_conv_grad_f32), and the dense adjoints finish:

    [dW1; dW2] = dP' x          (gnnmp_dense_grad_w_f32)         db = colsum(dP[:, :out])      dW = [dW1 | dW2]
    dx         = dP [W1; W2]    (gnnmp_dense_f32, W read transposed)

Nothing of E rows is written in either direction.  max / min hand Δ to EVERY maximiser (NNlib's rule); relu' is 0 at 0.
torch allocates and concatenates; every arithmetic step is a libgnnmp call.  `gnnmp.edge_conv` / `EdgeConv.__call__` (the reference's
literal composition, any nn) are unchanged.
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib as L
from .backward import _act_code, dense_grad_w, dense_grad_x, plan_transposed
from .graph import GNNGraph, check_num_nodes
from .msgpass import aggr_code


def stacked_weights(nn):
    """([W1; W2] [2 out][in], [b; 0] [2 out] | None) of nn = Dense(2 in => out): the column blocks of the weight stacked so that one
    contraction gives both shares of P (memory plumbing, cached per parameter version, as CGConv.split_weights)"""
    ps = (nn.weight, nn.bias)
    key = tuple((p.data_ptr(), p._version) for p in ps if p is not None)
    if getattr(nn, "_edge_stack_key", None) != key:
        W = nn.weight.detach()
        D = W.shape[1] // 2
        Wst = torch.cat([W[:, :D], W[:, D:]], dim=0).contiguous()
        bst = None if nn.bias is None else torch.cat([nn.bias.detach(), torch.zeros_like(nn.bias)]).contiguous()
        nn._edge_stack = (Wst, bst)
        nn._edge_stack_key = key
    return nn._edge_stack


def edge_conv_rows(plan, P, aggr, act, C):
    """y [N][C] of gnnmp_edge_conv_f32 on P [N][2C]"""
    y = torch.empty((P.shape[0], C), dtype=torch.float32, device=P.device)
    job = L.EdgeConvJob(L.ptr(P), L.ptr(y), aggr, act)
    L.check(L.load().gnnmp_edge_conv_f32(plan.handle, ctypes.byref(job), C, L.stream_ptr()))
    return y


def edge_conv_rows_grad(plan, plan_t, P, y, dy, aggr, act, C):
    """dP [N][2C] of gnnmp_edge_conv_grad_f32"""
    dP = torch.empty_like(P)
    job = L.EdgeConvGradJob(L.ptr(P), L.ptr(y), L.ptr(dy), L.ptr(dP), aggr, act)
    L.check(L.load().gnnmp_edge_conv_grad_f32(plan.handle, plan_t.handle, ctypes.byref(job), C, L.stream_ptr()))
    return dP


class _EdgeConvFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, Wst, bst, g, aggr, act):
        from .layers import dense
        x = x.contiguous()
        P = dense(x, Wst, bst)
        y = edge_conv_rows(g.plan(False), P, aggr, act, Wst.shape[0] // 2)
        ctx.save_for_backward(x, P, y, Wst)
        ctx.g, ctx.aggr, ctx.act, ctx.has_bias = g, aggr, act, bias is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, P, y, Wst = ctx.saved_tensors
        g = ctx.g
        C, D = y.shape[1], x.shape[1]
        dP = edge_conv_rows_grad(g.plan(False), plan_transposed(g, False), P, y, dy.contiguous(), ctx.aggr, ctx.act, C)
        dW = db = dx = None
        need_b = ctx.has_bias and ctx.needs_input_grad[2]
        if ctx.needs_input_grad[1] or need_b:
            dWst, dbst = dense_grad_w(dP, x, need_w=ctx.needs_input_grad[1], need_b=need_b)
            if dWst is not None:
                dW = torch.cat([dWst[:C], dWst[C:]], dim=1)          # [dW1 | dW2]: a copy, no arithmetic
            if dbst is not None:
                db = dbst[:C].contiguous()                           # colsum(dP[:, :C]); the second half belongs to the zeros under b
        if ctx.needs_input_grad[0]:
            dx = dense_grad_x(dP, Wst)
        return dx, dW, db, None, None, None, None, None


def edge_conv_ad(l, g: GNNGraph, x):
    """differentiable EdgeConv forward for a one-layer nn = Dense(2 in => out, identity | relu): gradients w.r.t. x, l.nn.weight,
    l.nn.bias.  Under torch.no_grad() it is simply the fused forward."""
    from .layers import Dense
    if isinstance(x, (tuple, list)):
        raise NotImplementedError("edge_conv_ad: a bipartite (xs, xt) input is not covered; pass one feature matrix")
    layers = list(l.nn) if isinstance(l.nn, (list, tuple)) else [l.nn]
    if len(layers) != 1:
        raise NotImplementedError(f"edge_conv_ad covers a one-layer nn (Dense(2 in => out, σ)), not {len(layers)} layers: per-edge layers "
                                  "after the first need edge-level adjoints; use gnnmp.edge_conv for the forward")
    nn = layers[0]
    if not isinstance(nn, Dense):
        raise NotImplementedError(f"edge_conv_ad: nn must be a gnnmp Dense, not {type(nn).__name__}")
    act = _act_code(nn.sigma)                  # ValueError unless identity / relu
    aggr = aggr_code(l.aggr)
    check_num_nodes(g, x)
    if nn.weight.shape[1] != 2 * x.shape[1]:
        raise ValueError(f"edge_conv_ad: nn must be Dense(2 in => out): its weight has {nn.weight.shape[1]} columns, x {x.shape[1]} features")
    Wst, bst = stacked_weights(nn)
    return _EdgeConvFn.apply(x, nn.weight, nn.bias, Wst, bst, g, aggr, act)
