"""NNConv, differentiable: the edge-conditioned convolution of MPNN trained on libgnnmp — forward as gnnmp.nn_conv, pullback on the
one-pass per-edge-matrix adjoint.

nn_conv (GNNlib/src/layers/conv.jl:260-273) is σ.(weight * x .+ m .+ bias) with m = propagate(W_k x_j, g, aggr) and
W_k = reshape(nn(e)_k, out, in).  Three differentiable pieces, chained by torch:

    we = nn(e)              [E][out * in]    gnnmp.Dense layers, each through dense_ad: the E-row adjoints are the existing dense adjoints
    m  = aggregate(x, we)   [N][out]         forward gnnmp_propagate_nn_f32; backward gnnmp_nn_conv_grad_f32 (csrc/nn_grad.hip) on the
                                             transposed plan: dwe [E][out * in] = Δ_i ⊗ x_j and dx = Σ_k W_k' Δ_i in ONE walk that reads we
                                             once and writes dwe once.  `mean` pre-scales Δ by 1 / indeg (gnnmp_mul_rows_f32).
    y  = σ.(weight * x .+ m .+ bias)         dense, _add, bias_act; backward act_grad, dense_grad_w, dense_grad_x; Δm = Δz

torch allocates and sums the two contributions to dx; every other arithmetic step is a libgnnmp call.  What needs_input_grad says is not
needed is not computed: if neither e nor a parameter of nn needs a gradient no E x out x in buffer is allocated.  `gnnmp.nn_conv` /
`NNConv.__call__` are unchanged; under torch.no_grad() nn_conv_ad gives their bits.
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib as L
from .backward import _in_count, act_grad, dense_ad, dense_grad_w, dense_grad_x, plan_transposed
from .graph import GNNGraph, check_num_edges, check_num_nodes
from .layers import Dense, bias_act, dense
from .layers_more import _add
from .msgpass import aggr_code


def nn_rows_grad(plan_t, x, we, dm, Din, Dout, want_x=True, want_we=True):
    """(dx | None, dwe | None) of gnnmp_nn_conv_grad_f32; `we` is not read (and may be None) when dx is not wanted"""
    dx = torch.empty_like(x) if want_x else None
    dwe = torch.empty((plan_t.n_edges, Dout * Din), dtype=torch.float32, device=x.device) if want_we else None
    job = L.NNConvGradJob(L.ptr(x), L.ptr(we) if want_x else None, L.ptr(dm), L.ptr(dx), L.ptr(dwe))
    L.check(L.load().gnnmp_nn_conv_grad_f32(plan_t.handle, ctypes.byref(job), Din, Dout, L.stream_ptr()))
    return dx, dwe


class _NNAggregateFn(torch.autograd.Function):
    """(x, we) -> m = aggr_{k: j -> i} W_k x_j"""

    @staticmethod
    def forward(ctx, x, we, g, aggr):
        nin = x.shape[1]
        out = we.shape[1] // nin
        m = torch.empty((g.num_nodes, out), dtype=torch.float32, device=x.device)
        L.check(L.load().gnnmp_propagate_nn_f32(g.plan(False).handle, aggr_code(aggr), L.ptr(x), L.ptr(we), L.ptr(m), nin, out,
                                                L.stream_ptr()))
        ctx.save_for_backward(x, we)
        ctx.g, ctx.mean = g, aggr_code(aggr) == L.MEAN
        return m

    @staticmethod
    def backward(ctx, dm):
        x, we = ctx.saved_tensors
        g = ctx.g
        need_x, need_we = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_x or need_we):
            return None, None, None, None
        dm = dm.contiguous()
        nin, out = x.shape[1], dm.shape[1]
        if ctx.mean:
            inv = 1.0 / _in_count(g, False).clamp(min=1.0)      # N-element host-side plumbing, as propagate_grad_xj
            scaled = torch.empty_like(dm)
            L.check(L.load().gnnmp_mul_rows_f32(L.ptr(inv), 1, L.ptr(dm), L.ptr(scaled), dm.shape[0], out, L.stream_ptr()))
            dm = scaled
        dx, dwe = nn_rows_grad(plan_transposed(g, False), x, we, dm, nin, out, want_x=need_x, want_we=need_we)
        return dx, dwe, None, None


class _NNTailFn(torch.autograd.Function):
    """(x, m, weight, bias) -> σ.(weight * x .+ m .+ bias)"""

    @staticmethod
    def forward(ctx, x, m, weight, bias, sigma):
        y = bias_act(_add(dense(x, weight), m), bias, sigma)
        ctx.save_for_backward(x, weight, y)
        ctx.sigma, ctx.has_bias = sigma, bias is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, y = ctx.saved_tensors
        dz = act_grad(dy.contiguous(), y, ctx.sigma)
        dW, db = dense_grad_w(dz, x, need_w=ctx.needs_input_grad[2], need_b=ctx.has_bias and ctx.needs_input_grad[3])
        dx = dense_grad_x(dz, weight) if ctx.needs_input_grad[0] else None
        return dx, (dz if ctx.needs_input_grad[1] else None), dW, db, None


def nn_conv_ad(l, g: GNNGraph, x, e):
    """differentiable NNConv forward: gradients w.r.t. x, e, l.weight, l.bias and the weights and biases of l.nn (a gnnmp.Dense or a list of
    them); aggr + or mean, σ identity or relu.  Under torch.no_grad() it is gnnmp.nn_conv, bit for bit."""
    if isinstance(x, (tuple, list)):
        raise NotImplementedError("nn_conv_ad: a bipartite (xs, xt) input is not covered; pass one feature matrix")
    if aggr_code(l.aggr) not in (L.SUM, L.MEAN):
        raise NotImplementedError(f"nn_conv_ad: aggr = {l.aggr!r} is not covered; the adjoint exists for + and mean")
    layers = list(l.nn) if isinstance(l.nn, (list, tuple)) else [l.nn]
    for k, layer in enumerate(layers):
        if not isinstance(layer, Dense):
            raise TypeError(f"nn_conv_ad: layer {k} of nn is a {type(layer).__name__}; the adjoint covers gnnmp.Dense layers only")
    check_num_nodes(g, x)
    check_num_edges(g, e)
    out, nin = l.weight.shape
    if x.shape[1] != nin:
        raise ValueError(f"nn_conv_ad: x has {x.shape[1]} features, the layer was built for {nin}")
    x = x.contiguous()
    we = e.contiguous()
    for layer in layers:
        we = dense_ad(layer, we)
    if we.shape[1] != out * nin:
        raise ValueError(f"nn_conv_ad: nn(e) has {we.shape[1]} features, the layer needs out * in = {out * nin}")
    m = _NNAggregateFn.apply(x, we.contiguous(), g, l.aggr)
    return _NNTailFn.apply(x, m, l.weight, l.bias, l.sigma)
