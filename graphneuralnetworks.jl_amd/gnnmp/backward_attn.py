"""Differentiable GATv2Conv and TransformerConv (attention core + root weight + skip connection) — forward AND backward on
the HIP kernels (csrc/gat_fused.hip, csrc/attn_backward.hip), wrapped as torch.autograd.Functions like gnnmp/backward.py.
The forward keeps 8 bytes of softmax statistics per destination and head; the pullback is two edge passes that rebuild α in
registers, then the dense adjoints.  concat = true or false (mean over heads and its pullback as two leaf kernels).  With edge
features (`e`, GATv2Conv's dense_e / TransformerConv's W6) forward and pullback run on csrc/attn_edge.hip, which also writes the
gradient dF of the per-edge row F = dense_e(e) | W6(e), one store per edge; de and the edge weights follow by the dense adjoints on E
rows.  No dropout together with `e`."""
from __future__ import annotations

import torch

from . import _lib as L
from .backward import _act_code, act_grad, dense_grad_w, dense_grad_x, plan_transposed
from .graph import GNNGraph, check_num_edges, check_num_nodes
from .layers import dense
from .layers_attn import ATTN_DOT, ATTN_GATV2, SELF_LOOPS_MSG, check_edge_row_width


def _attn_forward(plan, mode, Q, K, V, a, slope, scale, bias, act, H, C, p_drop=0.0, seed=0):
    N = plan.n_dst
    out = torch.empty((N, H * C), dtype=torch.float32, device=K.device)
    stats = torch.empty((N, H, 2), dtype=torch.float32, device=K.device)
    if p_drop > 0.0:
        L.check(L.load().gnnmp_attn_conv_drop_f32(plan.handle, mode, L.ptr(Q), L.ptr(K), L.ptr(V), L.ptr(a), float(slope),
                                                  float(scale), float(p_drop), int(seed), L.ptr(bias), act, L.ptr(out),
                                                  L.ptr(stats), H, C, L.stream_ptr()))
    else:
        L.check(L.load().gnnmp_attn_conv_f32(plan.handle, mode, L.ptr(Q), L.ptr(K), L.ptr(V), L.ptr(a), float(slope), float(scale),
                                             L.ptr(bias), act, L.ptr(out), L.ptr(stats), H, C, L.stream_ptr()))
    return out, stats


def _attn_backward(g, loops, mode, Q, K, V, a, slope, scale, stats, dz, H, C, p_drop=0.0, seed=0):
    plan, plan_t = g.plan(loops), plan_transposed(g, loops)
    N = g.num_nodes
    f32 = dict(dtype=torch.float32, device=dz.device)
    line = torch.empty((N, H, 4), **f32)
    dQ = torch.empty((N, H * C), **f32)
    dK = torch.empty((N, H * C), **f32)
    dV = torch.empty((N, H * C), **f32) if mode == ATTN_DOT else None
    dA = torch.empty((N, H * C), **f32) if mode == ATTN_GATV2 else None
    da = torch.empty((H, C), **f32) if mode == ATTN_GATV2 else None
    if p_drop > 0.0:
        L.check(L.load().gnnmp_attn_conv_grad_drop_f32(plan.handle, plan_t.handle, mode, L.ptr(Q), L.ptr(K), L.ptr(V), L.ptr(a),
                                                       float(slope), float(scale), float(p_drop), int(seed), L.ptr(stats), L.ptr(dz),
                                                       L.ptr(line), L.ptr(dQ), L.ptr(dK), L.ptr(dV), L.ptr(dA), L.ptr(da), H, C,
                                                       L.stream_ptr()))
    else:
        L.check(L.load().gnnmp_attn_conv_grad_f32(plan.handle, plan_t.handle, mode, L.ptr(Q), L.ptr(K), L.ptr(V), L.ptr(a),
                                                  float(slope), float(scale), L.ptr(stats), L.ptr(dz), L.ptr(line), L.ptr(dQ),
                                                  L.ptr(dK), L.ptr(dV), L.ptr(dA), L.ptr(da), H, C, L.stream_ptr()))
    return dQ, dK, dV, da


def _attn_edge_forward(plan, mode, Q, K, V, F, a, slope, scale, bias, act, H, C):
    N = plan.n_dst
    out = torch.empty((N, H * C), dtype=torch.float32, device=K.device)
    stats = torch.empty((N, H, 2), dtype=torch.float32, device=K.device)
    job = L.AttnEdgeJob(L.ptr(Q), L.ptr(K), L.ptr(V), L.ptr(F), L.ptr(a), L.ptr(bias), L.ptr(out), L.ptr(stats), float(slope),
                        float(scale), int(act))
    L.check(L.load().gnnmp_attn_conv_edge_f32(plan.handle, mode, job, H, C, L.stream_ptr()))
    return out, stats


def _attn_edge_backward(g, mode, Q, K, V, F, a, slope, scale, stats, dz, H, C, need_da=True):
    """(dQ, dK, dV | None, dF, da | None) of gnnmp_attn_conv_edge_grad_f32; the plans carry no self loops"""
    plan, plan_t = g.plan(False), plan_transposed(g, False)
    N = g.num_nodes
    f32 = dict(dtype=torch.float32, device=dz.device)
    line = torch.empty((N, H, 4), **f32)
    dQ, dK, dF = torch.empty((N, H * C), **f32), torch.empty((N, H * C), **f32), torch.empty(F.shape, **f32)
    dV = torch.empty((N, H * C), **f32) if mode == ATTN_DOT else None
    dA = torch.empty((N, H * C), **f32) if mode == ATTN_GATV2 else None
    da = torch.empty((H, C), **f32) if (mode == ATTN_GATV2 and need_da) else None
    job = L.AttnEdgeGradJob(L.ptr(Q), L.ptr(K), L.ptr(V), L.ptr(F), L.ptr(a), L.ptr(stats), L.ptr(dz), L.ptr(line), L.ptr(dQ), L.ptr(dK),
                            L.ptr(dV), L.ptr(dF), L.ptr(dA), L.ptr(da), float(slope), float(scale))
    L.check(L.load().gnnmp_attn_conv_edge_grad_f32(plan.handle, plan_t.handle, mode, job, H, C, L.stream_ptr()))
    return dQ, dK, dV, dF, da


def _add_(a, b):
    L.check(L.load().gnnmp_add_f32(L.ptr(a), L.ptr(b), L.ptr(a), a.numel(), L.stream_ptr()))
    return a


class _GATv2ConvFn(torch.autograd.Function):
    """gatv2_conv (GNNlib/src/layers/conv.jl:171-214), e === nothing; concat = true or false"""

    @staticmethod
    def forward(ctx, x, Wi, bi, Wj, a, bias, g, sigma, heads, slope, loops, concat=True, p_drop=0.0, seed=0):
        H, C = heads, Wi.shape[0] // heads
        x = x.contiguous()
        Q = dense(x, Wi, bi)
        K = dense(x, Wj)
        a_hc = a.t().contiguous()                                   # (C, H) as Julia stores it -> [H][C]
        # concat = false: heads averaged before bias and σ (conv.jl:196-200): the kernel's fused tail is off
        out, stats = _attn_forward(g.plan(loops), ATTN_GATV2, Q, K, None, a_hc, slope, 1.0, bias if concat else None,
                                   _act_code(sigma) if concat else L.ACT_IDENTITY, H, C, p_drop, seed)
        ctx.p_drop, ctx.seed = float(p_drop), int(seed)
        if not concat:
            y = torch.empty((out.shape[0], C), dtype=torch.float32, device=x.device)
            L.check(L.load().gnnmp_head_mean_f32(L.ptr(out), L.ptr(bias), _act_code(sigma), L.ptr(y), out.shape[0], H, C,
                                                 L.stream_ptr()))
            out = y
        ctx.save_for_backward(x, Wi, Wj, Q, K, a_hc, stats, out)
        ctx.g, ctx.sigma, ctx.H, ctx.C, ctx.slope, ctx.loops, ctx.concat = g, sigma, H, C, slope, loops, concat
        ctx.has_bi, ctx.has_b = bi is not None, bias is not None
        return out

    @staticmethod
    def backward(ctx, dy):
        x, Wi, Wj, Q, K, a_hc, stats, y = ctx.saved_tensors
        dz = act_grad(dy.contiguous(), y, ctx.sigma)
        db = dense_grad_w(dz, dz, need_w=False)[1] if ctx.has_b else None
        if not ctx.concat:                       # pullback of mean(x, dims = 2): every head receives Δ / H
            dzh = torch.empty((dz.shape[0], ctx.H * ctx.C), dtype=torch.float32, device=dz.device)
            L.check(L.load().gnnmp_head_mean_grad_f32(L.ptr(dz), L.ptr(dzh), dz.shape[0], ctx.H, ctx.C, L.stream_ptr()))
            dz = dzh
        dQ, dK, _, da = _attn_backward(ctx.g, ctx.loops, ATTN_GATV2, Q, K, None, a_hc, ctx.slope, 1.0, stats, dz, ctx.H, ctx.C,
                                       ctx.p_drop, ctx.seed)
        dWi, dbi = dense_grad_w(dQ, x, need_b=ctx.has_bi)
        dWj, _ = dense_grad_w(dK, x, need_b=False)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = _add_(dense_grad_x(dQ, Wi), dense_grad_x(dK, Wj))
        return dx, dWi, dbi, dWj, da.t(), db, None, None, None, None, None, None, None, None


class _GATv2ConvEdgeFn(torch.autograd.Function):
    """gatv2_conv (conv.jl:171-214) with e: the edge row F = dense_e(e) inside the logit; concat = true or false"""

    @staticmethod
    def forward(ctx, x, e, Wi, bi, Wj, We, a, bias, g, sigma, heads, slope, concat):
        H, C = heads, Wi.shape[0] // heads
        x, e = x.contiguous(), e.contiguous()
        Q, K, F = dense(x, Wi, bi), dense(x, Wj), dense(e, We)
        a_hc = a.t().contiguous()
        out, stats = _attn_edge_forward(g.plan(False), ATTN_GATV2, Q, K, None, F, a_hc, slope, 1.0, bias if concat else None,
                                        _act_code(sigma) if concat else L.ACT_IDENTITY, H, C)
        if not concat:
            y = torch.empty((out.shape[0], C), dtype=torch.float32, device=x.device)
            L.check(L.load().gnnmp_head_mean_f32(L.ptr(out), L.ptr(bias), _act_code(sigma), L.ptr(y), out.shape[0], H, C,
                                                 L.stream_ptr()))
            out = y
        ctx.save_for_backward(x, e, Wi, Wj, We, Q, K, F, a_hc, stats, out)
        ctx.g, ctx.sigma, ctx.H, ctx.C, ctx.slope, ctx.concat = g, sigma, H, C, slope, concat
        ctx.has_bi, ctx.has_b = bi is not None, bias is not None
        return out

    @staticmethod
    def backward(ctx, dy):
        x, e, Wi, Wj, We, Q, K, F, a_hc, stats, y = ctx.saved_tensors
        need = ctx.needs_input_grad
        dz = act_grad(dy.contiguous(), y, ctx.sigma)
        db = dense_grad_w(dz, dz, need_w=False)[1] if (ctx.has_b and need[7]) else None
        if not ctx.concat:
            dzh = torch.empty((dz.shape[0], ctx.H * ctx.C), dtype=torch.float32, device=dz.device)
            L.check(L.load().gnnmp_head_mean_grad_f32(L.ptr(dz), L.ptr(dzh), dz.shape[0], ctx.H, ctx.C, L.stream_ptr()))
            dz = dzh
        dQ, dK, _, dF, da = _attn_edge_backward(ctx.g, ATTN_GATV2, Q, K, None, F, a_hc, ctx.slope, 1.0, stats, dz, ctx.H, ctx.C,
                                                need_da=need[6])
        dWi, dbi = dense_grad_w(dQ, x, need_w=need[2], need_b=ctx.has_bi and need[3])
        dWj = dense_grad_w(dK, x, need_b=False)[0] if need[4] else None
        dWe = dense_grad_w(dF, e, need_b=False)[0] if need[5] else None
        dx = _add_(dense_grad_x(dQ, Wi), dense_grad_x(dK, Wj)) if need[0] else None
        de = dense_grad_x(dF, We) if need[1] else None
        return dx, de, dWi, dbi, dWj, dWe, None if da is None else da.t(), db, None, None, None, None, None


def _check_edge_args(l, e, has_edge_weight, what, H, C):
    """the reference's assertions on e (conv.jl:173-174, 178-181) and this path's own refusals, by name, before any C call"""
    assert not (e is None and has_edge_weight), "Input edge features required for this layer"
    assert not (e is not None and not has_edge_weight), "Input edge features were not specified in the layer constructor"
    if e is not None:
        assert not l.add_self_loops, SELF_LOOPS_MSG
        assert float(getattr(l, "dropout", 0.0)) == 0.0, f"{what}: attention dropout together with edge features is not supported"
        check_edge_row_width(H, C, f"{what} with edge features")


def gatv2_conv_ad(l, g: GNNGraph, x, e=None, seed=None):
    """differentiable GATv2Conv forward: gradients w.r.t. x, dense_i (weight, bias), dense_j weight, a, bias — and, with edge features,
    e and dense_e's weight.  l.dropout > 0 (without e): the attention coefficients are dropped (conv.jl:191) with the mask of `seed`
    (default: the layer's next one), regenerated in the pullback"""
    check_num_nodes(g, x)
    _check_edge_args(l, e, l.dense_e_weight is not None, "GATv2Conv", l.heads, l.channel[1])
    if e is not None:
        check_num_edges(g, e)
        return _GATv2ConvEdgeFn.apply(x, e, l.dense_i_weight, l.dense_i_bias, l.dense_j_weight, l.dense_e_weight, l.a, l.bias, g,
                                      l.sigma, l.heads, l.negative_slope, bool(l.concat))
    p_drop = float(getattr(l, "dropout", 0.0))
    if p_drop > 0.0:
        if seed is None:
            seed = l.next_seed()
        l.last_seed = int(seed)
    return _GATv2ConvFn.apply(x, l.dense_i_weight, l.dense_i_bias, l.dense_j_weight, l.a, l.bias, g, l.sigma, l.heads,
                              l.negative_slope, bool(l.add_self_loops), bool(l.concat), p_drop, 0 if seed is None else int(seed))


class _TransformerConvFn(torch.autograd.Function):
    """transformer_conv (conv.jl:553-629): attention core, + W1 x (root weight), + x (skip connection); concat = true"""

    @staticmethod
    def forward(ctx, x, W1, b1, W2, b2, W3, b3, W4, b4, g, heads, sqrt_out, loops, skip, concat=True):
        H, C = heads, W2.shape[0] // heads
        x = x.contiguous()
        V, Q, K = dense(x, W2, b2), dense(x, W3, b3), dense(x, W4, b4)
        h, stats = _attn_forward(g.plan(loops), ATTN_DOT, Q, K, V, None, 0.0, sqrt_out, None, L.ACT_IDENTITY, H, C)
        if not concat:                                              # mean over heads before the root weight (conv.jl:600-603)
            y = torch.empty((h.shape[0], C), dtype=torch.float32, device=x.device)
            L.check(L.load().gnnmp_head_mean_f32(L.ptr(h), None, L.ACT_IDENTITY, L.ptr(y), h.shape[0], H, C, L.stream_ptr()))
            h = y
        ctx.concat = concat
        if W1 is not None:
            _add_(h, dense(x, W1, b1))
        if skip:
            _add_(h, x)
        ctx.save_for_backward(x, Q, K, V, stats, W2, W3, W4, *([W1] if W1 is not None else []))
        ctx.g, ctx.H, ctx.C, ctx.scale, ctx.loops, ctx.skip = g, H, C, sqrt_out, loops, skip
        ctx.has = (W1 is not None, b1 is not None, b2 is not None, b3 is not None, b4 is not None)
        return h

    @staticmethod
    def backward(ctx, dy):
        x, Q, K, V, stats, W2, W3, W4, *rest = ctx.saved_tensors
        W1 = rest[0] if rest else None
        dh = dy.contiguous()
        dha = dh
        if not ctx.concat:
            dha = torch.empty((dh.shape[0], ctx.H * ctx.C), dtype=torch.float32, device=dh.device)
            L.check(L.load().gnnmp_head_mean_grad_f32(L.ptr(dh), L.ptr(dha), dh.shape[0], ctx.H, ctx.C, L.stream_ptr()))
        dQ, dK, dV, _ = _attn_backward(ctx.g, ctx.loops, ATTN_DOT, Q, K, V, None, 0.0, ctx.scale, stats, dha, ctx.H, ctx.C)
        has_w1, hb1, hb2, hb3, hb4 = ctx.has
        dW2, db2 = dense_grad_w(dV, x, need_b=hb2)
        dW3, db3 = dense_grad_w(dQ, x, need_b=hb3)
        dW4, db4 = dense_grad_w(dK, x, need_b=hb4)
        dW1 = db1 = None
        if has_w1:
            dW1, db1 = dense_grad_w(dh, x, need_b=hb1)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = dense_grad_x(dV, W2)
            _add_(dx, dense_grad_x(dQ, W3))
            _add_(dx, dense_grad_x(dK, W4))
            if has_w1:
                _add_(dx, dense_grad_x(dh, W1))
            if ctx.skip:
                _add_(dx, dh)
        return dx, dW1, db1, dW2, db2, dW3, db3, dW4, db4, None, None, None, None, None, None


class _AGNNConvFn(torch.autograd.Function):
    """agnn_conv (conv.jl:337-352) as the reference writes it — xn = x ./ norm, α = softmax(β (xn_i . xn_j)), Σ α x_j — so
    that the pullback is the dot-product attention pullback on (Q, K, V) = (xn, xn, x) plus the row normalisation's:
      Δx = ΔV + ∇normalise(ΔQ + ΔK),   Δβ = Σ_e Δlogit_e cos_e = (1 / β) Σ_i xn_i . ΔQ_i   (ΔQ_i = β Σ_e Δlogit_e xn_j)"""

    @staticmethod
    def forward(ctx, x, beta, g, loops):
        x = x.contiguous()
        N, D = x.shape
        b = float(beta)
        assert b != 0.0, "β = 0 makes every logit zero: Δβ is not recoverable from ΔQ (use a non-zero init_beta)"
        lib = L.load()
        xn = torch.empty_like(x)
        rn = torch.empty(N, dtype=torch.float32, device=x.device)
        L.check(lib.gnnmp_row_normalize_f32(L.ptr(x), L.ptr(xn), L.ptr(rn), N, D, L.stream_ptr()))
        out, stats = _attn_forward(g.plan(loops), ATTN_DOT, xn, xn, x, None, 0.0, 1.0 / b, None, L.ACT_IDENTITY, 1, D)
        ctx.save_for_backward(x, xn, rn, stats)
        ctx.g, ctx.loops, ctx.b = g, loops, b
        return out

    @staticmethod
    def backward(ctx, dy):
        x, xn, rn, stats = ctx.saved_tensors
        N, D = x.shape
        dQ, dK, dV, _ = _attn_backward(ctx.g, ctx.loops, ATTN_DOT, xn, xn, x, None, 0.0, 1.0 / ctx.b, stats, dy.contiguous(), 1, D)
        dx = torch.empty_like(x)
        qdot = torch.empty((N, 1), dtype=torch.float32, device=x.device)
        L.check(L.load().gnnmp_row_normalize_grad_f32(L.ptr(dQ), L.ptr(dK), L.ptr(xn), L.ptr(rn), L.ptr(dV), L.ptr(dx),
                                                      L.ptr(qdot), 1.0 / ctx.b, N, D, L.stream_ptr()))
        dbeta = None
        if ctx.needs_input_grad[1]:
            dbeta = dense_grad_w(qdot, qdot, need_w=False)[1]                   # deterministic column sum of (N, 1)
        return dx, dbeta, None, None


def agnn_conv_ad(l, g: GNNGraph, x):
    """differentiable AGNNConv forward: gradients w.r.t. x and β (when `l.beta` is a 1-element tensor that requires grad)"""
    check_num_nodes(g, x)
    beta = l.beta if torch.is_tensor(l.beta) else torch.tensor([float(l.beta)], dtype=torch.float32, device=x.device)
    return _AGNNConvFn.apply(x, beta, g, bool(l.add_self_loops))


class _TransformerConvEdgeFn(torch.autograd.Function):
    """transformer_conv (conv.jl:553-629) with e: W6 e inside the key and the value, + W1 x (root weight), + x (skip connection)"""

    @staticmethod
    def forward(ctx, x, e, W1, b1, W2, b2, W3, b3, W4, b4, W6, b6, g, heads, sqrt_out, skip, concat):
        H, C = heads, W2.shape[0] // heads
        x, e = x.contiguous(), e.contiguous()
        V, Q, K, F = dense(x, W2, b2), dense(x, W3, b3), dense(x, W4, b4), dense(e, W6, b6)
        h, stats = _attn_edge_forward(g.plan(False), ATTN_DOT, Q, K, V, F, None, 0.0, sqrt_out, None, L.ACT_IDENTITY, H, C)
        if not concat:
            y = torch.empty((h.shape[0], C), dtype=torch.float32, device=x.device)
            L.check(L.load().gnnmp_head_mean_f32(L.ptr(h), None, L.ACT_IDENTITY, L.ptr(y), h.shape[0], H, C, L.stream_ptr()))
            h = y
        if W1 is not None:
            _add_(h, dense(x, W1, b1))
        if skip:
            _add_(h, x)
        ctx.save_for_backward(x, e, Q, K, V, F, stats, W2, W3, W4, W6, *([W1] if W1 is not None else []))
        ctx.g, ctx.H, ctx.C, ctx.scale, ctx.skip, ctx.concat = g, H, C, sqrt_out, skip, concat
        ctx.has = (W1 is not None, b1 is not None, b2 is not None, b3 is not None, b4 is not None, b6 is not None)
        return h

    @staticmethod
    def backward(ctx, dy):
        x, e, Q, K, V, F, stats, W2, W3, W4, W6, *rest = ctx.saved_tensors
        W1 = rest[0] if rest else None
        need = ctx.needs_input_grad
        dh = dy.contiguous()
        dha = dh
        if not ctx.concat:
            dha = torch.empty((dh.shape[0], ctx.H * ctx.C), dtype=torch.float32, device=dh.device)
            L.check(L.load().gnnmp_head_mean_grad_f32(L.ptr(dh), L.ptr(dha), dh.shape[0], ctx.H, ctx.C, L.stream_ptr()))
        dQ, dK, dV, dF, _ = _attn_edge_backward(ctx.g, ATTN_DOT, Q, K, V, F, None, 0.0, ctx.scale, stats, dha, ctx.H, ctx.C)
        has_w1, hb1, hb2, hb3, hb4, hb6 = ctx.has
        dW1, db1 = dense_grad_w(dh, x, need_w=need[2], need_b=hb1 and need[3]) if has_w1 else (None, None)
        dW2, db2 = dense_grad_w(dV, x, need_w=need[4], need_b=hb2 and need[5])
        dW3, db3 = dense_grad_w(dQ, x, need_w=need[6], need_b=hb3 and need[7])
        dW4, db4 = dense_grad_w(dK, x, need_w=need[8], need_b=hb4 and need[9])
        dW6, db6 = dense_grad_w(dF, e, need_w=need[10], need_b=hb6 and need[11])
        dx = None
        if need[0]:
            dx = dense_grad_x(dV, W2)
            _add_(dx, dense_grad_x(dQ, W3))
            _add_(dx, dense_grad_x(dK, W4))
            if has_w1:
                _add_(dx, dense_grad_x(dh, W1))
            if ctx.skip:
                _add_(dx, dh)
        de = dense_grad_x(dF, W6) if need[1] else None
        return dx, de, dW1, db1, dW2, db2, dW3, db3, dW4, db4, dW6, db6, None, None, None, None, None


def transformer_conv_ad(l, g: GNNGraph, x, e=None):
    """differentiable TransformerConv forward (concat = true or false): gradients w.r.t. x and W1..W4 (+ their biases) — and, with edge
    features, e and W6 (+ its bias)"""
    check_num_nodes(g, x)
    _check_edge_args(l, e, l.W6_weight is not None, "TransformerConv", l.heads, l.channels[1])
    if e is not None:
        check_num_edges(g, e)
        return _TransformerConvEdgeFn.apply(x, e, l.W1_weight, l.W1_bias, l.W2_weight, l.W2_bias, l.W3_weight, l.W3_bias, l.W4_weight,
                                            l.W4_bias, l.W6_weight, l.W6_bias, g, l.heads, l.sqrt_out, bool(l.skip_connection),
                                            bool(l.concat))
    return _TransformerConvFn.apply(x, l.W1_weight, l.W1_bias, l.W2_weight, l.W2_bias, l.W3_weight, l.W3_bias, l.W4_weight,
                                    l.W4_bias, g, l.heads, l.sqrt_out, bool(l.add_self_loops), bool(l.skip_connection),
                                    bool(l.concat))
