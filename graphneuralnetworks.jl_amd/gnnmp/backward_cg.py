"""CGConv, differentiable: the first layer with edge features that can be trained on libgnnmp — forward as gnnmp.cg_conv, pullback on the
fused gated-message adjoint.

cg_conv (GNNlib/src/layers/conv.jl:304-333) is propagate(cg_message, g, +) with the message dense_f(z) .* dense_s(z), z = vcat(xi, xj, e).
The column blocks of [Wf; Ws] turn the two contractions on E rows into three dense calls (gnnmp.cg_conv, layers_more.py):

    fs_i = x [Wf_i; Ws_i]' + [bf; bs]   [N][2 out]      fs_j = x [Wf_j; Ws_j]'   [N][2 out]      fs_e = e [Wf_e; Ws_e]'   [E][2 out]

and gnnmp_propagate_cg_f32 does the per-edge sum, sigmoid, act, product and + in one pass.  The pullback has the mirrored shape:
gnnmp_cg_conv_grad_f32 (csrc/cg_grad.hip; one pass over the plan, one over the transposed plan) recomputes the pre-activations and gives
dfs_i, dfs_j [N][2 out] and — only if e or the weights need a gradient — dfs_e [E][2 out]; the dense adjoints finish:

    d[Wf_i; Ws_i] = dfs_i' x,  [dbf; dbs] = colsum(dfs_i)     d[Wf_j; Ws_j] = dfs_j' x     d[Wf_e; Ws_e] = dfs_e' e    (gnnmp_dense_grad_w_f32)
    dx = dfs_i [Wf_i; Ws_i] + dfs_j [Wf_j; Ws_j] (+ Δ if the residual was applied)          de = dfs_e [Wf_e; Ws_e]      (gnnmp_dense_f32)
    dWf = [dWf_i | dWf_j | dWf_e],  dWs likewise: copies

torch allocates, slices and concatenates; every arithmetic step is a libgnnmp call.  What needs_input_grad says is not needed is not
computed.  `gnnmp.cg_conv` / `CGConv.__call__` are unchanged; under torch.no_grad() cg_conv_ad gives their bits.
"""
from __future__ import annotations

import ctypes
import warnings

import torch

from . import _lib as L
from .backward import dense_grad_w, dense_grad_x, plan_transposed
from .graph import GNNGraph, check_num_edges, check_num_nodes
from .layers_more import _CG_ACT, _add


def cg_rows_grad(plan, plan_t, fs_i, fs_j, fs_e, dy, act, C, want_e):
    """(dfs_i, dfs_j, dfs_e | None) of gnnmp_cg_conv_grad_f32"""
    dfs_i, dfs_j = torch.empty_like(fs_i), torch.empty_like(fs_j)
    dfs_e = torch.empty_like(fs_e) if want_e and fs_e is not None else None
    job = L.CGConvGradJob(L.ptr(fs_i), L.ptr(fs_j), L.ptr(fs_e), L.ptr(dy), L.ptr(dfs_i), L.ptr(dfs_j), L.ptr(dfs_e), act)
    L.check(L.load().gnnmp_cg_conv_grad_f32(plan.handle, plan_t.handle, ctypes.byref(job), C, L.stream_ptr()))
    return dfs_i, dfs_j, dfs_e


class _CGConvFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, e, Wf, Ws, bf, bs, l, g):
        from .layers import dense
        out = l.ch[1]
        x = x.contiguous()
        e = e.contiguous() if e is not None else None
        Wi, Wj, We, b = l.split_weights()
        fs_i = dense(x, Wi, b)
        fs_j = dense(x, Wj)
        fs_e = dense(e, We) if e is not None else None
        m = torch.empty((g.num_nodes, out), dtype=torch.float32, device=x.device)
        L.check(L.load().gnnmp_propagate_cg_f32(g.plan(False).handle, L.ptr(fs_i), L.ptr(fs_j), L.ptr(fs_e), _CG_ACT[l.act], L.ptr(m), out,
                                                L.stream_ptr()))
        ctx.residual = l.residual and x.shape[1] == out
        if ctx.residual:
            m = _add(m, x)
        empty = torch.empty(0, device=x.device)
        ctx.save_for_backward(x, e if e is not None else empty, fs_i, fs_j, fs_e if fs_e is not None else empty, Wi, Wj,
                              We if We is not None else empty)
        ctx.g, ctx.act, ctx.has_e, ctx.has_bias = g, _CG_ACT[l.act], e is not None, bf is not None
        return m

    @staticmethod
    def backward(ctx, dy):
        x, e, fs_i, fs_j, fs_e, Wi, Wj, We = ctx.saved_tensors
        g = ctx.g
        C = fs_i.shape[1] // 2
        need_x, need_e = ctx.needs_input_grad[0], ctx.has_e and ctx.needs_input_grad[1]
        need_w = ctx.needs_input_grad[2] or ctx.needs_input_grad[3]
        need_b = ctx.has_bias and (ctx.needs_input_grad[4] or ctx.needs_input_grad[5])
        if not (need_x or need_e or need_w or need_b):
            return (None,) * 8
        dy = dy.contiguous()
        if not ctx.has_e:
            e = fs_e = We = None
        dfs_i, dfs_j, dfs_e = cg_rows_grad(g.plan(False), plan_transposed(g, False), fs_i, fs_j, fs_e, dy, ctx.act, C,
                                           want_e=need_e or need_w)
        dx = de = dWf = dWs = dbf = dbs = None
        if need_w or need_b:
            dWi, db = dense_grad_w(dfs_i, x, need_w=need_w, need_b=need_b)
            if need_w:
                blocks = [dWi, dense_grad_w(dfs_j, x, need_b=False)[0]]
                if ctx.has_e:
                    blocks.append(dense_grad_w(dfs_e, e, need_b=False)[0])
                if ctx.needs_input_grad[2]:
                    dWf = torch.cat([blk[:C] for blk in blocks], dim=1)      # [dWf_i | dWf_j | dWf_e]: a copy, no arithmetic
                if ctx.needs_input_grad[3]:
                    dWs = torch.cat([blk[C:] for blk in blocks], dim=1)
            if need_b:
                dbf = db[:C].contiguous() if ctx.needs_input_grad[4] else None
                dbs = db[C:].contiguous() if ctx.needs_input_grad[5] else None
        if need_x:
            dx = _add(dense_grad_x(dfs_i, Wi), dense_grad_x(dfs_j, Wj))
            if ctx.residual:
                dx = _add(dx, dy)
        if need_e:
            de = dense_grad_x(dfs_e, We)
        return dx, de, dWf, dWs, dbf, dbs, None, None


def cg_conv_ad(l, g: GNNGraph, x, e=None):
    """differentiable CGConv forward: gradients w.r.t. x, e, l.dense_f_weight, l.dense_s_weight, l.dense_f_bias, l.dense_s_bias.  Under
    torch.no_grad() it is gnnmp.cg_conv, bit for bit."""
    if isinstance(x, (tuple, list)):
        raise NotImplementedError("cg_conv_ad: a bipartite (xs, xt) input is not covered; pass one feature matrix")
    check_num_nodes(g, x)
    (nin, ein), out = l.ch
    if x.shape[1] != nin:
        raise ValueError(f"cg_conv_ad: x has {x.shape[1]} features, the layer was built for {nin}")
    if e is not None:
        check_num_edges(g, e)
        if ein == 0:
            raise ValueError("cg_conv_ad: the layer was built without edge features (ein = 0), but e was given")
        if e.shape[1] != ein:
            raise ValueError(f"cg_conv_ad: e has {e.shape[1]} features, the layer was built for {ein}")
    elif ein != 0:
        raise ValueError("cg_conv_ad: CGConv was built with edge features, but e is missing")
    if l.residual and nin != out:
        warnings.warn("number of output features different from number of input features, residual not applied.")
    return _CGConvFn.apply(x, e, l.dense_f_weight, l.dense_s_weight, l.dense_f_bias, l.dense_s_bias, l, g)
