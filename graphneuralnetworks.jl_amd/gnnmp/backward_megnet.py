"""MEGNetConv, differentiable: the one layer that updates the edge features and returns them, trained on libgnnmp — forward and pullback
on the fused edge-update kernels — and the pullback of aggregate_neighbors for all four folds.

megnet_conv (GNNlib/src/layers/conv.jl:356-368), edge k: j -> i.  W0 = [A | B | D] is ϕe's first weight, split at columns in and 2 in; its
column blocks turn the x part of the first ϕe layer into two dense calls on the N node rows (include/gnnmp.h states the arithmetic,
csrc/megnet.hip holds the kernels).  Four differentiable pieces, chained by torch:

    edge head    P = x A' + b0, Q = x B'  [N][hid],  F = e D'  [E][hid]                                        gnnmp_dense_f32
                 a0_k = σ0((P_i + Q_j) + F_k)                                                                  gnnmp_megnet_edge_f32
                 pullback: dz0 = Δa0 ⊙ σ0'(z0), dP = Σ_in dz0, dQ = Σ_out dz0                                  gnnmp_megnet_edge_grad_f32
                 dA = dP' x, db0 = colsum(dP), dB = dQ' x, dD = dz0' e, dx = dP A + dQ B, de = dz0 D           dense_grad_w / dense_grad_x
    rest of ϕe   gnnmp.Dense layers through dense_ad -> ē
    edge output  ē -> (ē, xᵉ = aggregate_neighbors(g, aggr, ē)); pullback: ONE gnnmp_aggregate_grad_f32 call that adds the cotangent
                 of the returned ē to the scatter's pullback (acc) — no separate add; acc = None when the caller uses only x̄
    node head    σ.(W [x | xᵉ]' .+ b) as the two-segment dense call; pullback act_grad, dense_grad_w2, dense_grad_x; then dense_ad

No [E][in] gather of x exists in either direction.  torch allocates, slices, concatenates and chains; every arithmetic step is a libgnnmp
call.  What needs_input_grad says is not needed is not computed: dz0 [E][hid] is not stored when neither e nor W0 needs a gradient.
SAVED BY THE EDGE HEAD: for σ0 = relu (the default) a0 itself serves as z (the mask z0 > 0 is the mask a0 > 0) and for identity nothing
is needed, so no z0 is written; softplus, tanh and swish keep z0.

The fused forward reassociates the first layer — (P_i + Q_j) + F_k with the bias inside P, where gnnmp.megnet_conv adds the bias last:
megnet_conv_ad owes gnnmp.megnet_conv and the oracle the 1e-5 bar, NOT equal bits.  `gnnmp.megnet_conv` / `MEGNetConv.__call__` are
unchanged.
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib as L
from .backward import _act_code, act_grad, dense_ad, dense_grad_w, dense_grad_w2, dense_grad_x, plan_transposed
from .graph import GNNGraph, check_num_edges, check_num_nodes
from .layers import Dense, dense
from .layers_more import _ACT_CODES, _add
from .msgpass import _scatter_plan, aggr_code

_RELU_CALLABLES = (torch.relu, torch.nn.functional.relu)


def _p(t):
    """the device pointer, NULL for None and for an empty tensor"""
    return None if t is None or t.numel() == 0 else L.ptr(t)


def megnet_edge(plan, P, Q, F, act, want_z0=False):
    """(a0 [E][hid], z0 [E][hid] | None) of gnnmp_megnet_edge_f32; F [E][hid] | None"""
    N, hid = P.shape
    a0 = torch.empty((plan.n_total, hid), dtype=torch.float32, device=P.device)
    z0 = torch.empty_like(a0) if want_z0 else None
    job = L.MegnetEdgeJob(_p(P), _p(Q), _p(F), _p(a0), _p(z0), act)
    if N > 0 and plan.n_total > 0:      # (an empty tensor has no address: nothing to launch, nothing to refuse)
        L.check(L.load().gnnmp_megnet_edge_f32(plan.handle, ctypes.byref(job), hid, L.stream_ptr()))
    return a0, z0


def megnet_edge_grad(plan, plan_t, da0, z, act, want_dz0=True, want_nodes=True):
    """(dz0 [E][hid] | None, dP, dQ [N][hid] | None) of gnnmp_megnet_edge_grad_f32; z: the pre-activation (None for identity; a0 will do
    for relu)"""
    hid = da0.shape[1]
    dz0 = torch.empty_like(da0) if want_dz0 else None
    dP = torch.empty((plan.n_dst, hid), dtype=torch.float32, device=da0.device) if want_nodes else None
    dQ = torch.empty_like(dP) if want_nodes else None
    if not (want_dz0 or want_nodes) or plan.n_dst == 0 or (plan.n_total == 0 and not want_nodes):
        return dz0, dP, dQ
    job = L.MegnetEdgeGradJob(_p(da0), _p(z), _p(dz0), _p(dP), _p(dQ), act)
    L.check(L.load().gnnmp_megnet_edge_grad_f32(plan.handle, plan_t.handle if want_nodes else None, ctypes.byref(job), hid, L.stream_ptr()))
    return dz0, dP, dQ


def aggregate_grad(plan, aggr, dy, m=None, y=None, acc=None):
    """dm [E][D] of gnnmp_aggregate_grad_f32: the pullback of scatter(aggr, m, t) (+ acc); m and y are read for max / min only"""
    code = aggr_code(aggr)
    D = dy.shape[1]
    dm = torch.empty((plan.n_total, D), dtype=torch.float32, device=dy.device)
    if plan.n_dst > 0 and plan.n_total > 0:
        sel = code in (L.MAX, L.MIN)
        job = L.AggregateGradJob(_p(dy), _p(m) if sel else None, _p(y) if sel else None, _p(acc), _p(dm))
        L.check(L.load().gnnmp_aggregate_grad_f32(plan.handle, ctypes.byref(job), code, D, L.stream_ptr()))
    return dm


class _AggregateFn(torch.autograd.Function):
    """m [E][D] -> aggregate_neighbors(g, aggr, m)"""

    @staticmethod
    def forward(ctx, m, g, aggr):
        plan = g.plan(False)
        y = _scatter_plan(aggr, m, plan)
        sel = aggr_code(aggr) in (L.MAX, L.MIN)
        ctx.save_for_backward(*((m, y) if sel else ()))
        ctx.g, ctx.aggr = g, aggr
        return y

    @staticmethod
    def backward(ctx, dy):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        m, y = ctx.saved_tensors if ctx.saved_tensors else (None, None)
        return aggregate_grad(ctx.g.plan(False), ctx.aggr, dy.contiguous(), m, y), None, None


def aggregate_neighbors_ad(g: GNNGraph, aggr, m):
    """differentiable aggregate_neighbors (msgpass.jl:145-149) for +, mean, max, min on [E][D] float32 messages: the forward is
    gnnmp.aggregate_neighbors bit for bit, the backward NNlib's scatter pullback (max / min: every tying copy gets the whole Δ)"""
    check_num_edges(g, m)
    aggr_code(aggr)
    if m.dim() != 2 or m.dtype != torch.float32:
        raise ValueError(f"aggregate_neighbors_ad: m must be a float32 [E][D] matrix, not {tuple(m.shape)} {m.dtype}")
    return _AggregateFn.apply(m.contiguous(), g, aggr)


class _EdgeHeadFn(torch.autograd.Function):
    """(x, e, W0, b0) -> a0 = σ0((P_i + Q_j) + F_k)"""

    @staticmethod
    def forward(ctx, x, e, W0, b0, g, act):
        nin = x.shape[1]
        P = dense(x, W0[:, :nin], b0)
        Q = dense(x, W0[:, nin:2 * nin])
        F = dense(e, W0[:, 2 * nin:]) if e.shape[0] > 0 else None
        keep = any(ctx.needs_input_grad[:4])
        a0, z0 = megnet_edge(g.plan(False), P, Q, F, act, keep and act not in (L.ACT_IDENTITY, L.ACT_RELU))
        if keep:
            z = a0 if act == L.ACT_RELU else z0
            ctx.save_for_backward(x, e, W0, *(() if z is None else (z,)))
        ctx.g, ctx.act, ctx.has_bias = g, act, b0 is not None
        return a0

    @staticmethod
    def backward(ctx, da0):
        x, e, W0, *rest = ctx.saved_tensors
        z = rest[0] if rest else None
        g, nin = ctx.g, x.shape[1]
        need_x, need_e, need_w = ctx.needs_input_grad[:3]
        need_b = ctx.has_bias and ctx.needs_input_grad[3]
        want_dz0, want_nodes = need_e or need_w, need_x or need_w or need_b
        dz0, dP, dQ = megnet_edge_grad(g.plan(False), plan_transposed(g, False) if want_nodes else None, da0.contiguous(), z, ctx.act,
                                       want_dz0, want_nodes)
        dx = de = dW0 = db0 = None
        if need_w or need_b:
            dA, db0 = dense_grad_w(dP, x, need_w=need_w, need_b=need_b)
        if need_w:
            dW0 = torch.cat([dA, dense_grad_w(dQ, x, need_b=False)[0], dense_grad_w(dz0, e, need_b=False)[0]], dim=1)   # [dA | dB | dD]
        if need_x:
            dx = _add(dense_grad_x(dP, W0[:, :nin]), dense_grad_x(dQ, W0[:, nin:2 * nin]))
        if need_e:
            de = dense_grad_x(dz0, W0[:, 2 * nin:])
        return dx, de, dW0, db0, None, None


class _EdgeOutFn(torch.autograd.Function):
    """ē -> (ē, xᵉ = aggregate_neighbors(g, aggr, ē)); the pullback sums both cotangents of ē inside gnnmp_aggregate_grad_f32"""

    @staticmethod
    def forward(ctx, eb, g, aggr):
        ctx.set_materialize_grads(False)
        xe = _scatter_plan(aggr, eb, g.plan(False))
        sel = aggr_code(aggr) in (L.MAX, L.MIN)
        ctx.save_for_backward(*((eb, xe) if sel else ()))
        ctx.g, ctx.aggr = g, aggr
        return eb, xe

    @staticmethod
    def backward(ctx, deb, dxe):
        if not ctx.needs_input_grad[0] or (deb is None and dxe is None):
            return None, None, None
        if dxe is None:
            return deb, None, None
        m, y = ctx.saved_tensors if ctx.saved_tensors else (None, None)
        acc = None if deb is None else deb.contiguous()
        return aggregate_grad(ctx.g.plan(False), ctx.aggr, dxe.contiguous(), m, y, acc), None, None


class _NodeHeadFn(torch.autograd.Function):
    """(x, xᵉ, W, b) -> σ.(W [x | xᵉ]' .+ b), ϕv's first layer as the two-segment dense call"""

    @staticmethod
    def forward(ctx, x, xe, W, b, sigma):
        nin = x.shape[1]
        y = dense(x, W[:, :nin], b, sigma, x2=xe, W2=W[:, nin:])
        ctx.save_for_backward(x, xe, W, y)
        ctx.sigma, ctx.has_bias = sigma, b is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, xe, W, y = ctx.saved_tensors
        nin = x.shape[1]
        need_x, need_xe, need_w = ctx.needs_input_grad[:3]
        need_b = ctx.has_bias and ctx.needs_input_grad[3]
        dz = act_grad(dy.contiguous(), y, ctx.sigma)
        dW = db = None
        if need_w:
            both = dense_grad_w2(dz, x, xe)      # one read of dz; None outside that entry point's envelope (in % 16 != 0)
            if both is None:
                dW1, db = dense_grad_w(dz, x, need_b=need_b)
                both = (dW1, dense_grad_w(dz, xe, need_b=False)[0], db)
            dW, db = torch.cat([both[0], both[1]], dim=1), (both[2] if need_b else None)      # [dW_x | dW_xe]: a copy
        elif need_b:
            db = dense_grad_w(dz, x, need_w=False, need_b=True)[1]
        dx = dense_grad_x(dz, W[:, :nin]) if need_x else None
        dxe = dense_grad_x(dz, W[:, nin:]) if need_xe else None
        return dx, dxe, dW, db, None


def _act0(sigma):
    """the gnnmp_act code of ϕe's first layer: any of the five"""
    if sigma in _RELU_CALLABLES:
        return L.ACT_RELU
    if callable(sigma) or sigma not in _ACT_CODES:
        raise ValueError(f"megnet_conv_ad: the first ϕe layer's σ = {sigma!r} is not in the gnnmp_act set (identity, relu, softplus, "
                         "tanh, swish)")
    return _ACT_CODES[sigma]


def megnet_conv_ad(l, g: GNNGraph, x, e):
    """differentiable MEGNetConv forward -> (x̄, ē): gradients w.r.t. x, e and every weight and bias of l.phi_e and l.phi_v, for all four
    aggr.  ϕe's first layer takes any σ of the gnnmp_act set (identity | relu | softplus | tanh | swish), every other layer identity or
    relu.  The fused first layer is summed as (P_i + Q_j) + F_k: the outputs agree with gnnmp.megnet_conv and the oracle to the 1e-5
    bar, not bit for bit."""
    if isinstance(x, (tuple, list)):
        raise NotImplementedError("megnet_conv_ad: a bipartite (xs, xt) input is not covered; pass one feature matrix")
    pe, pv = list(l.phi_e), list(l.phi_v)
    for name, chain in (("phi_e", pe), ("phi_v", pv)):
        if not chain:
            raise ValueError(f"megnet_conv_ad: {name} is empty")
        for k, layer in enumerate(chain):
            if not isinstance(layer, Dense):
                raise TypeError(f"megnet_conv_ad: layer {k} of {name} is a {type(layer).__name__}; the adjoint covers gnnmp.Dense layers only")
    act0 = _act0(pe[0].sigma)
    for name, chain in (("phi_e", pe[1:]), ("phi_v", pv)):
        for layer in chain:
            try:
                _act_code(layer.sigma)
            except ValueError:
                raise ValueError(f"megnet_conv_ad: σ = {layer.sigma!r} in {name}; beyond ϕe's first layer the adjoints cover identity and "
                                 "relu") from None
    aggr_code(l.aggr)
    check_num_nodes(g, x)
    check_num_edges(g, e)
    if x.dim() != 2 or e.dim() != 2:
        raise ValueError(f"megnet_conv_ad: x and e must be matrices, not {tuple(x.shape)} and {tuple(e.shape)}")
    nin, ein = x.shape[1], e.shape[1]
    W0, Wv = pe[0].weight, pv[0].weight
    if W0.shape[1] != 2 * nin + ein:
        raise ValueError(f"megnet_conv_ad: the first ϕe weight has {W0.shape[1]} columns, 2 in + ein = {2 * nin + ein} are needed "
                         f"(x has {nin} features, e has {ein})")
    out_e = pe[-1].weight.shape[0]
    if Wv.shape[1] != nin + out_e:
        raise ValueError(f"megnet_conv_ad: the first ϕv weight has {Wv.shape[1]} columns, in + (ϕe's output) = {nin + out_e} are needed")
    x, e = x.contiguous(), e.contiguous()
    eb = _EdgeHeadFn.apply(x, e, W0, pe[0].bias, g, act0)
    for layer in pe[1:]:
        eb = dense_ad(layer, eb)
    eb, xe = _EdgeOutFn.apply(eb, g, l.aggr)
    xb = _NodeHeadFn.apply(x, xe, Wv, pv[0].bias, pv[0].sigma)
    for layer in pv[1:]:
        xb = dense_ad(layer, xb)
    return xb, eb
