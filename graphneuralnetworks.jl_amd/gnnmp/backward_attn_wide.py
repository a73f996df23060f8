"""Differentiable GATConv, GATv2Conv and TransformerConv on feature rows WIDER than a wave (heads * out > 256: 8 x 64, 4 x 128,
4 x 256 ...) — forward and pullback on the head-tiled kernels of csrc/attn_wide.hip (include/gnnmp.h: gnnmp_attn_conv_wide_f32,
gnnmp_attn_conv_wide_grad_f32), wrapped as torch.autograd.Functions like gnnmp/backward_attn.py.  gat_conv_ad, gatv2_conv_ad and
transformer_conv_ad come here when the row does not fit one wave, a head does, there is no `e` and no attention dropout; the tails
(head mean, bias and σ, root weight, skip connection) and the dense adjoints are the narrow paths' own calls."""
from __future__ import annotations

import torch

from . import _lib as L
from .backward import _act_code, act_grad, dense_grad_w, dense_grad_x, plan_transposed
from .backward_attn import _add_
from .layers import dense
from .layers_attn import ATTN_DOT, ATTN_GAT, ATTN_GATV2


def _wide_forward(plan, mode, Q, K, V, a, slope, scale, bias, act, H, C):
    N = plan.n_dst
    out = torch.empty((N, H * C), dtype=torch.float32, device=K.device)
    stats = torch.empty((N, H, 2), dtype=torch.float32, device=K.device)
    job = L.AttnWideJob(L.ptr(Q), L.ptr(K), L.ptr(V), L.ptr(a), L.ptr(bias), L.ptr(out), L.ptr(stats), float(slope), float(scale),
                        int(act))
    L.check(L.load().gnnmp_attn_conv_wide_f32(plan.handle, mode, job, H, C, L.stream_ptr()))
    return out, stats


def _wide_backward(g, loops, mode, Q, K, V, a, slope, scale, stats, dz, H, C, need_da=True):
    """(dQ, dK, dV | None, da | None) of gnnmp_attn_conv_wide_grad_f32; Q None: dK is the whole gradient of K"""
    plan, plan_t = g.plan(loops), plan_transposed(g, loops)
    N = g.num_nodes
    f32 = dict(dtype=torch.float32, device=dz.device)
    line, dQ, dK = torch.empty((N, H, 4), **f32), torch.empty((N, H * C), **f32), torch.empty((N, H * C), **f32)
    dV = torch.empty((N, H * C), **f32) if mode == ATTN_DOT else None
    dA = None if mode == ATTN_DOT else torch.empty(((2 if mode == ATTN_GAT else 1) * N, H * C), **f32)
    da = None if mode == ATTN_DOT or not need_da else torch.empty((H, (2 if mode == ATTN_GAT else 1) * C), **f32)
    job = L.AttnWideGradJob(L.ptr(Q), L.ptr(K), L.ptr(V), L.ptr(a), L.ptr(stats), L.ptr(dz), L.ptr(line), L.ptr(dQ), L.ptr(dK), L.ptr(dV),
                            L.ptr(dA), L.ptr(da), float(slope), float(scale))
    L.check(L.load().gnnmp_attn_conv_wide_grad_f32(plan.handle, plan_t.handle, mode, job, H, C, L.stream_ptr()))
    return dQ, dK, dV, da


def _head_mean(out, bias, code, H, C):
    y = torch.empty((out.shape[0], C), dtype=torch.float32, device=out.device)
    L.check(L.load().gnnmp_head_mean_f32(L.ptr(out), L.ptr(bias), code, L.ptr(y), out.shape[0], H, C, L.stream_ptr()))
    return y


def _head_mean_grad(dz, H, C):
    """pullback of mean(x, dims = 2): every head receives Δ / H"""
    dzh = torch.empty((dz.shape[0], H * C), dtype=torch.float32, device=dz.device)
    L.check(L.load().gnnmp_head_mean_grad_f32(L.ptr(dz), L.ptr(dzh), dz.shape[0], H, C, L.stream_ptr()))
    return dzh


class _GATConvWideFn(torch.autograd.Function):
    """gat_conv (GNNlib/src/layers/conv.jl:112-167), no edge features, no dropout; concat = true or false"""

    @staticmethod
    def forward(ctx, x, weight, a, bias, g, sigma, heads, slope, loops, concat):
        H, C = heads, weight.shape[0] // heads
        x = x.contiguous()
        Wx = dense(x, weight)
        a_hc = a.t().contiguous()                                   # [H][2C]
        # concat = false: the heads are averaged BEFORE bias and σ (conv.jl:143-147), so the kernel's fused tail is off
        out, stats = _wide_forward(g.plan(loops), ATTN_GAT, None, Wx, None, a_hc, slope, 1.0, bias if concat else None,
                                   _act_code(sigma) if concat else L.ACT_IDENTITY, H, C)
        if not concat:
            out = _head_mean(out, bias, _act_code(sigma), H, C)
        ctx.save_for_backward(x, weight, Wx, a_hc, stats, out)
        ctx.g, ctx.sigma, ctx.H, ctx.C, ctx.slope, ctx.loops, ctx.concat, ctx.has_b = g, sigma, H, C, slope, loops, concat, bias is not None
        return out

    @staticmethod
    def backward(ctx, dy):
        x, weight, Wx, a_hc, stats, y = ctx.saved_tensors
        need = ctx.needs_input_grad
        dz = act_grad(dy.contiguous(), y, ctx.sigma)
        db = dense_grad_w(dz, dz, need_w=False)[1] if (ctx.has_b and need[3]) else None
        if not ctx.concat:
            dz = _head_mean_grad(dz, ctx.H, ctx.C)
        _, dWx, _, da = _wide_backward(ctx.g, ctx.loops, ATTN_GAT, None, Wx, None, a_hc, ctx.slope, 1.0, stats, dz, ctx.H, ctx.C,
                                       need_da=need[2])
        dW = dense_grad_w(dWx, x, need_b=False)[0] if need[1] else None
        dx = dense_grad_x(dWx, weight) if need[0] else None
        return dx, dW, None if da is None else da.t(), db, None, None, None, None, None, None


class _GATv2ConvWideFn(torch.autograd.Function):
    """gatv2_conv (conv.jl:171-214), e === nothing, no dropout; concat = true or false"""

    @staticmethod
    def forward(ctx, x, Wi, bi, Wj, a, bias, g, sigma, heads, slope, loops, concat):
        H, C = heads, Wi.shape[0] // heads
        x = x.contiguous()
        Q, K = dense(x, Wi, bi), dense(x, Wj)
        a_hc = a.t().contiguous()                                   # (C, H) as Julia stores it -> [H][C]
        out, stats = _wide_forward(g.plan(loops), ATTN_GATV2, Q, K, None, a_hc, slope, 1.0, bias if concat else None,
                                   _act_code(sigma) if concat else L.ACT_IDENTITY, H, C)
        if not concat:
            out = _head_mean(out, bias, _act_code(sigma), H, C)
        ctx.save_for_backward(x, Wi, Wj, Q, K, a_hc, stats, out)
        ctx.g, ctx.sigma, ctx.H, ctx.C, ctx.slope, ctx.loops, ctx.concat = g, sigma, H, C, slope, loops, concat
        ctx.has_bi, ctx.has_b = bi is not None, bias is not None
        return out

    @staticmethod
    def backward(ctx, dy):
        x, Wi, Wj, Q, K, a_hc, stats, y = ctx.saved_tensors
        need = ctx.needs_input_grad
        dz = act_grad(dy.contiguous(), y, ctx.sigma)
        db = dense_grad_w(dz, dz, need_w=False)[1] if (ctx.has_b and need[5]) else None
        if not ctx.concat:
            dz = _head_mean_grad(dz, ctx.H, ctx.C)
        dQ, dK, _, da = _wide_backward(ctx.g, ctx.loops, ATTN_GATV2, Q, K, None, a_hc, ctx.slope, 1.0, stats, dz, ctx.H, ctx.C,
                                       need_da=need[4])
        dWi, dbi = dense_grad_w(dQ, x, need_w=need[1], need_b=ctx.has_bi and need[2])
        dWj = dense_grad_w(dK, x, need_b=False)[0] if need[3] else None
        dx = _add_(dense_grad_x(dQ, Wi), dense_grad_x(dK, Wj)) if need[0] else None
        return dx, dWi, dbi, dWj, None if da is None else da.t(), db, None, None, None, None, None, None


class _TransformerConvWideFn(torch.autograd.Function):
    """transformer_conv (conv.jl:553-629) without e: attention core, [mean over heads], + W1 x (root weight), + x (skip connection)"""

    @staticmethod
    def forward(ctx, x, W1, b1, W2, b2, W3, b3, W4, b4, g, heads, sqrt_out, loops, skip, concat):
        H, C = heads, W2.shape[0] // heads
        x = x.contiguous()
        V, Q, K = dense(x, W2, b2), dense(x, W3, b3), dense(x, W4, b4)
        h, stats = _wide_forward(g.plan(loops), ATTN_DOT, Q, K, V, None, 0.0, sqrt_out, None, L.ACT_IDENTITY, H, C)
        if not concat:                                              # mean over heads before the root weight (conv.jl:600-603)
            h = _head_mean(h, None, L.ACT_IDENTITY, H, C)
        if W1 is not None:
            _add_(h, dense(x, W1, b1))
        if skip:
            _add_(h, x)
        ctx.save_for_backward(x, Q, K, V, stats, W2, W3, W4, *([W1] if W1 is not None else []))
        ctx.g, ctx.H, ctx.C, ctx.scale, ctx.loops, ctx.skip, ctx.concat = g, H, C, sqrt_out, loops, skip, concat
        ctx.has = (W1 is not None, b1 is not None, b2 is not None, b3 is not None, b4 is not None)
        return h

    @staticmethod
    def backward(ctx, dy):
        x, Q, K, V, stats, W2, W3, W4, *rest = ctx.saved_tensors
        W1 = rest[0] if rest else None
        need = ctx.needs_input_grad
        dh = dy.contiguous()
        dha = dh if ctx.concat else _head_mean_grad(dh, ctx.H, ctx.C)
        dQ, dK, dV, _ = _wide_backward(ctx.g, ctx.loops, ATTN_DOT, Q, K, V, None, 0.0, ctx.scale, stats, dha, ctx.H, ctx.C)
        has_w1, hb1, hb2, hb3, hb4 = ctx.has
        dW1, db1 = dense_grad_w(dh, x, need_w=need[1], need_b=hb1 and need[2]) if has_w1 else (None, None)
        dW2, db2 = dense_grad_w(dV, x, need_w=need[3], need_b=hb2 and need[4])
        dW3, db3 = dense_grad_w(dQ, x, need_w=need[5], need_b=hb3 and need[6])
        dW4, db4 = dense_grad_w(dK, x, need_w=need[7], need_b=hb4 and need[8])
        dx = None
        if need[0]:
            dx = dense_grad_x(dV, W2)
            _add_(dx, dense_grad_x(dQ, W3))
            _add_(dx, dense_grad_x(dK, W4))
            if has_w1:
                _add_(dx, dense_grad_x(dh, W1))
            if ctx.skip:
                _add_(dx, dh)
        return dx, dW1, db1, dW2, db2, dW3, db3, dW4, db4, None, None, None, None, None, None


def gat_conv_wide_ad(l, g, x):
    return _GATConvWideFn.apply(x, l.dense_x_weight, l.a, l.bias, g, l.sigma, l.heads, l.negative_slope, bool(l.add_self_loops),
                                bool(l.concat))


def gatv2_conv_wide_ad(l, g, x):
    return _GATv2ConvWideFn.apply(x, l.dense_i_weight, l.dense_i_bias, l.dense_j_weight, l.a, l.bias, g, l.sigma, l.heads,
                                  l.negative_slope, bool(l.add_self_loops), bool(l.concat))


def transformer_conv_wide_ad(l, g, x):
    return _TransformerConvWideFn.apply(x, l.W1_weight, l.W1_bias, l.W2_weight, l.W2_bias, l.W3_weight, l.W3_bias, l.W4_weight,
                                        l.W4_bias, g, l.heads, l.sqrt_out, bool(l.add_self_loops), bool(l.skip_connection),
                                        bool(l.concat))
