"""EGNNConv, differentiable: the one layer that reads the coordinates themselves, trained on libgnnmp — the first pullback here through
which a coordinate gets a gradient, and the first with swish.

egnn_conv (GNNlib/src/layers/conv.jl:459-495), edge k: j -> i.  W0 = [A | B | c | D] is ϕe's first weight, split at columns nin, 2 nin,
2 nin + 1; its column blocks turn the h part of the first ϕe layer into two dense calls on the N node rows (include/gnnmp.h states the
arithmetic, csrc/egnn.hip holds the kernels):

    P = h A' + b0  [N][hid]      Q = h B'  [N][hid]      F = e D'  [E][hid] (only with edge features)          gnnmp_dense_f32
    q_k = |x_i − x_j|²,  z0_k = P_i + Q_j + q_k c (+ F_k),  a0 = act0(z0)                                      gnnmp_egnn_edge_f32  (K1)
    mh = the rest of ϕe on a0,  mx = ϕx(mh)  [E][1]                                                            dense + bias_act, E rows
    h_aggr = scatter(+, mh)                                                                                    gnnmp_scatter_f32
    x'_i = x_i + (1 / deg_i) Σ_{k into i} mx_k n_k,  n_k = (x_i − x_j) / (sqrt(q_k) + 1e-6)                    gnnmp_egnn_coord_f32 (K2)
    h' = ϕh(h, h_aggr) with its first weight split as egnn_conv does, + h under the residual

No [E][nin] gather of h, no [q | e] concatenation, no [E][Dx] array.  The pullback mirrors it: ϕh's adjoints on N rows give dh and
dh_aggr; dmx = (n_k · Δx'_i) / deg_i (gnnmp_egnn_coord_grad_f32, first use); ϕx's and ϕe's adjoints on E rows, with
gnnmp_act_grad_z_f32 working from the PRE-activations (swish cannot be inverted from its output), give dz0; dP = scatter(+, dz0) over
the plan and dQ over the transposed plan; dq = dz0 c, dc = dz0' q, dD = dz0' e, de = dz0 D; dA, db0, dB and the rest of dh on N rows;
dx = Δx' + Σ_in dd − Σ_out dd (gnnmp_egnn_coord_grad_f32, second use).  Where q_k == 0 (a self loop, coincident points) the n-path terms
of the coordinate adjoint are defined as 0; the reference's AD gives Inf * 0 there.

torch allocates, slices and concatenates; every arithmetic step is a libgnnmp call.  What needs_input_grad says is not needed is not
computed.  SAVED FOR THE BACKWARD: the pre-activation and output of every E-row layer, plus q and mx [E] — for the default layer five
[E][hid] arrays: z0, the pre-activation and output of ϕe's second layer (the output is mh), and the pre-activation and output of ϕx's
first layer.  a0 is not kept: the backward recomputes it from z0 with gnnmp_bias_act_f32, whose device function K1 shares — the same bits.
Under torch.no_grad(), or when nothing requires a gradient, nothing is kept and z0 is not written.

The forward is NOT gnnmp.egnn_conv call for call (z0 is summed in another order, and biases are folded into the dense calls): it owes the
oracle the 1e-5 bar, not equal bits.  `gnnmp.egnn_conv` / `EGNNConv.__call__` are unchanged.
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib as L
from .backward import dense_grad_w, dense_grad_x, plan_transposed
from .graph import GNNGraph, check_num_edges, check_num_nodes
from .layers_more import _ACT_CODES, _add, _bias_act_code
from .msgpass import _gather, _scatter_plan

MAX_DX = 16


def egnn_edge(g, x, P, Q, F, c, act, want_z0):
    """(q [E], a0 [E][hid], z0 [E][hid] | None) of gnnmp_egnn_edge_f32"""
    E, hid = g.num_edges, P.shape[1]
    q = torch.empty(E, dtype=torch.float32, device=x.device)
    a0 = torch.empty((E, hid), dtype=torch.float32, device=x.device)
    z0 = torch.empty_like(a0) if want_z0 else None
    job = L.EgnnEdgeJob(L.ptr(g.s), L.ptr(g.t), g.idx_bytes, g.index_base, L.ptr(x), L.ptr(P), L.ptr(Q), L.ptr(F), L.ptr(c), L.ptr(q),
                        L.ptr(a0), L.ptr(z0), act)
    if E > 0:      # (an empty tensor has no address: nothing to launch, nothing to refuse)
        L.check(L.load().gnnmp_egnn_edge_f32(ctypes.byref(job), E, hid, x.shape[1], L.stream_ptr()))
    return q, a0, z0


def egnn_coord(plan, x, mx):
    """x' of gnnmp_egnn_coord_f32"""
    xo = torch.empty_like(x)
    job = L.EgnnCoordJob(L.ptr(x), L.ptr(mx), L.ptr(xo))
    L.check(L.load().gnnmp_egnn_coord_f32(plan.handle, ctypes.byref(job), x.shape[1], L.stream_ptr()))
    return xo


def egnn_coord_grad(plan, plan_t, x, dxo, mx=None, dq=None, want_dmx=False, want_dx=False):
    """(dmx [E] | None, dx [N][Dx] | None) of gnnmp_egnn_coord_grad_f32"""
    dmx = torch.empty(plan.n_total, dtype=torch.float32, device=x.device) if want_dmx else None
    dx = torch.empty_like(x) if want_dx else None
    job = L.EgnnCoordGradJob(L.ptr(x), L.ptr(dxo), L.ptr(mx), L.ptr(dq), L.ptr(dmx), L.ptr(dx))
    if not want_dx and plan.n_total == 0:
        return dmx, dx
    L.check(L.load().gnnmp_egnn_coord_grad_f32(plan.handle, None if plan_t is None else plan_t.handle, ctypes.byref(job), x.shape[1],
                                               L.stream_ptr()))
    return dmx, dx


def act_grad_z(dy, z, act):
    """dz = dy ⊙ act'(z) from the pre-activation (gnnmp_act_grad_z_f32); identity: dy itself"""
    if act == L.ACT_IDENTITY:
        return dy
    dz = torch.empty_like(dy)
    job = L.ActGradZJob(L.ptr(dy), L.ptr(z), L.ptr(dz), act)
    L.check(L.load().gnnmp_act_grad_z_f32(ctypes.byref(job), dy.numel(), L.stream_ptr()))
    return dz


def _dense_pre(inp, W, b, act, inp2=None, W2=None):
    """(pre-activation, output) of one Dense layer: the bias is folded into the dense call, the activation is gnnmp_bias_act_f32"""
    from .layers import dense
    pre = dense(inp, W, b, None, x2=inp2, W2=W2)
    return pre, (pre if act == L.ACT_IDENTITY else _bias_act_code(pre, None, _code_name(act)))


_NAMES = {v: k for k, v in _ACT_CODES.items() if k is not None}


def _code_name(code):
    return _NAMES[code]


def _chain_forward(layers, z, keep):
    """run (W, b, act) Dense layers on z; keep: [(input, pre-activation)] per layer"""
    for W, b, act in layers:
        pre, out = _dense_pre(z, W, b, _ACT_CODES[act])
        keep.append((z, pre))
        z = out
    return z


def _chain_backward(layers, kept, dy, need_param, need_input):
    """adjoints of _chain_forward, last layer first: ([(dW | None, db | None)] in layer order, d input | None)"""
    grads = [None] * len(layers)
    for n in range(len(layers) - 1, -1, -1):
        W, b, act = layers[n]
        inp, pre = kept[n]
        dz = act_grad_z(dy, pre, _ACT_CODES[act])
        grads[n] = dense_grad_w(dz, inp, need_w=need_param[n][0], need_b=need_param[n][1])
        dy = dense_grad_x(dz, W) if (n > 0 or need_input) and _needs_below(need_param, n, need_input) else None
        if dy is None:
            break
    return [gr if gr is not None else (None, None) for gr in grads], dy


def _needs_below(need_param, n, need_input):
    return need_input or any(w or b for w, b in need_param[:n])


def _forward(l, g, h, x, e, keep):
    """(h', x') and, when keep is a dict, everything the backward reads"""
    from .layers import dense
    nin = l.num_features["in"]
    (W0, b0, act0), rest = l.phi_e[0], l.phi_e[1:]
    act0 = _ACT_CODES[act0]
    want = keep is not None
    plan = g.plan(False)
    P = dense(h, W0[:, :nin], b0)
    Q = dense(h, W0[:, nin:2 * nin])
    F = dense(e, W0[:, 2 * nin + 1:]) if e is not None else None
    c = W0[:, 2 * nin].contiguous()                                       # a column of W0 as [hid]: a copy
    q, a0, z0 = egnn_edge(g, x, P, Q, F, c, act0, want)
    kept_e, kept_x, kept_h = [], [], []
    mh = _chain_forward(rest, a0, kept_e)
    mx = _chain_forward(l.phi_x, mh, kept_x)                              # [E][1]
    h_aggr = _scatter_plan("+", mh, plan)
    xo = egnn_coord(plan, x, mx)
    (Wh, bh, ah), resth = l.phi_h[0], l.phi_h[1:]
    pre_h, out_h = _dense_pre(h, Wh[:, :nin], bh, _ACT_CODES[ah], h_aggr, Wh[:, nin:])
    hn = _chain_forward(resth, out_h, kept_h)
    if l.residual:
        hn = _add(h, hn)
    if want:
        if kept_e:
            kept_e[0] = (None, kept_e[0][1])      # a0 is recomputed from z0 in the backward
        keep.update(q=q, z0=z0, c=c, mx=mx, h_aggr=h_aggr, pre_h=pre_h, kept_e=kept_e, kept_x=kept_x, kept_h=kept_h, act0=act0)
    return hn, xo


def _params(l):
    """the layer's weights and biases in a fixed order, with their (chain, layer, 0 = weight | 1 = bias) addresses"""
    out, where = [], []
    for name in ("phi_e", "phi_x", "phi_h"):
        for n, (W, b, _) in enumerate(getattr(l, name)):
            out.append(W)
            where.append((name, n, 0))
            if b is not None:
                out.append(b)
                where.append((name, n, 1))
    return out, where


class _EGNNConvFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, x, e, l, g, *params):
        keep = {}
        hn, xo = _forward(l, g, h, x, e, keep)
        ctx.l, ctx.g, ctx.keep, ctx.has_e = l, g, keep, e is not None
        ctx.save_for_backward(h, x, e if e is not None else torch.empty(0, device=h.device))
        return hn, xo

    @staticmethod
    def backward(ctx, dhn, dxo):
        h, x, e = ctx.saved_tensors
        l, g, k = ctx.l, ctx.g, ctx.keep
        if not ctx.has_e:
            e = None
        nin = l.num_features["in"]
        need_h, need_x, need_e = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.has_e and ctx.needs_input_grad[2]
        _, where = _params(l)
        need = {name: [[False, False] for _ in getattr(l, name)] for name in ("phi_e", "phi_x", "phi_h")}
        for (name, n, wb), flag in zip(where, ctx.needs_input_grad[5:]):
            need[name][n][wb] = bool(flag)
        any_of = lambda name: any(w or b for w, b in need[name])      # noqa: E731
        need_pe, need_px, need_ph = any_of("phi_e"), any_of("phi_x"), any_of("phi_h")
        need_z0 = need_pe or need_h or need_e or need_x               # everything at or below K1
        need_edges = need_z0 or need_px
        grads = {name: [(None, None)] * len(getattr(l, name)) for name in ("phi_e", "phi_x", "phi_h")}
        dh = dx = de = None
        dhn, dxo = dhn.contiguous(), dxo.contiguous()
        plan = g.plan(False)
        # ---- ϕh on N rows: dh (its own share) and dh_aggr ------------------------------------------------------------------------
        dh_aggr = None
        if need_ph or need_h or need_z0:
            (Wh, bh, ah), resth = l.phi_h[0], l.phi_h[1:]
            tail, d_out_h = _chain_backward(resth, k["kept_h"], dhn, need["phi_h"][1:], True)
            dz = act_grad_z(d_out_h, k["pre_h"], _ACT_CODES[ah])
            dWh = dbh = None
            if need["phi_h"][0][0] or need["phi_h"][0][1]:
                dW1, dbh = dense_grad_w(dz, h, need_w=need["phi_h"][0][0], need_b=need["phi_h"][0][1])
                if need["phi_h"][0][0]:
                    dWh = torch.cat([dW1, dense_grad_w(dz, k["h_aggr"], need_b=False)[0]], dim=1)      # [dWh_h | dWh_aggr]: a copy
            grads["phi_h"] = [(dWh, dbh)] + tail
            if need_h:
                dh = dense_grad_x(dz, Wh[:, :nin])
            if need_z0:
                dh_aggr = dense_grad_x(dz, Wh[:, nin:])
        if need_h and l.residual:
            dh = _add(dh, dhn)
        # ---- the E rows --------------------------------------------------------------------------------------------------------------
        if need_edges:
            dmx, _ = egnn_coord_grad(plan, None, x, dxo, want_dmx=True)
            grads["phi_x"], dmh = _chain_backward(l.phi_x, k["kept_x"], dmx.reshape(-1, 1), need["phi_x"], need_z0)
        if need_z0:
            dmh = _add(_gather(dh_aggr, g.t, g.index_base), dmh)
            (W0, b0, _), rest = l.phi_e[0], l.phi_e[1:]
            kept_e = k["kept_e"]
            if kept_e and (need["phi_e"][1][0] or need["phi_e"][1][1]):
                kept_e = [(_bias_act_code(k["z0"], None, _code_name(k["act0"])), kept_e[0][1])] + kept_e[1:]      # a0, recomputed
            tail, da0 = _chain_backward(rest, kept_e, dmh, need["phi_e"][1:], True)
            dz0 = act_grad_z(da0, k["z0"], k["act0"])
            dW0 = db0 = None
            need_w0, need_b0 = need["phi_e"][0]
            if need_h or need_w0 or need_b0:
                dP = _scatter_plan("+", dz0, plan)
                dQ = _scatter_plan("+", dz0, plan_transposed(g, False)) if need_h or need_w0 else None
                if need_w0 or need_b0:
                    dA, db0 = dense_grad_w(dP, h, need_w=need_w0, need_b=need_b0)
                if need_w0:
                    blocks = [dA, dense_grad_w(dQ, h, need_b=False)[0], dense_grad_w(dz0, k["q"].reshape(-1, 1), need_b=False)[0]]
                    if e is not None:
                        blocks.append(dense_grad_w(dz0, e, need_b=False)[0])
                    dW0 = torch.cat(blocks, dim=1)                        # [dA | dB | dc | dD]: a copy
                if need_h:
                    dh = _add(dh, _add(dense_grad_x(dP, W0[:, :nin]), dense_grad_x(dQ, W0[:, nin:2 * nin])))
            grads["phi_e"] = [(dW0, db0)] + tail
            if need_e:
                de = dense_grad_x(dz0, W0[:, 2 * nin + 1:])
            if need_x:
                dq = dense_grad_x(dz0, k["c"].reshape(-1, 1))             # dz0 c  [E][1]
                _, dx = egnn_coord_grad(plan, plan_transposed(g, False), x, dxo, mx=k["mx"], dq=dq, want_dx=True)
        out = [grads[name][n][wb] for name, n, wb in where]
        return (dh, dx, de, None, None, *out)


def egnn_conv_ad(l, g: GNNGraph, h, x, e=None):
    """differentiable EGNNConv forward -> (h', x'): gradients w.r.t. h, x, e and every weight and bias of l.phi_e, l.phi_x, l.phi_h, with
    any activation of the gnnmp_act set (identity | relu | softplus | tanh | swish) in any position.  For the backward it keeps the
    pre-activation and output of every E-row layer plus q and mx [E] — five [E][hid] arrays for the default layer (the module docstring
    names them); under torch.no_grad() nothing is kept and z0 is not written."""
    if isinstance(h, (tuple, list)):
        raise NotImplementedError("egnn_conv_ad: a bipartite (hs, ht) input is not covered; pass one feature matrix")
    check_num_nodes(g, h)
    check_num_nodes(g, x)
    nin, ein = l.num_features["in"], l.num_features["edge"]
    if h.shape[1] != nin:
        raise ValueError(f"egnn_conv_ad: h has {h.shape[1]} features, the layer was built for {nin}")
    if x.dim() != 2 or not 1 <= x.shape[1] <= MAX_DX:
        raise ValueError(f"egnn_conv_ad: x has {x.shape[-1]} coordinates per node; 1 .. {MAX_DX} are covered (Dx > {MAX_DX} is not)")
    if e is not None:
        check_num_edges(g, e)
        if ein == 0:
            raise ValueError("egnn_conv_ad: the layer was built without edge features (ein = 0), but e was given")
        if e.shape[1] != ein:
            raise ValueError(f"egnn_conv_ad: e has {e.shape[1]} features, the layer was built for {ein}")
    elif ein != 0:
        raise ValueError("egnn_conv_ad: EGNNConv was built with edge features, but e is missing")
    W0, Wh, Wx = l.phi_e[0][0], l.phi_h[0][0], l.phi_x[-1][0]
    if W0.shape[1] != 2 * nin + 1 + ein:
        raise ValueError(f"egnn_conv_ad: the first ϕe weight has {W0.shape[1]} columns, 2 in + 1 + ein = {2 * nin + 1 + ein} are needed")
    if Wh.shape[1] != nin + l.phi_e[-1][0].shape[0]:
        raise ValueError(f"egnn_conv_ad: the first ϕh weight has {Wh.shape[1]} columns, in + (ϕe's output) = "
                         f"{nin + l.phi_e[-1][0].shape[0]} are needed")
    if Wx.shape[0] != 1:
        raise ValueError(f"egnn_conv_ad: the last ϕx layer has {Wx.shape[0]} outputs; it must have 1 (one scale per edge)")
    for name in ("phi_e", "phi_x", "phi_h"):
        for _, _, act in getattr(l, name):
            if act not in _ACT_CODES:
                raise ValueError(f"egnn_conv_ad: activation {act!r} of {name} is not in the gnnmp_act set")
    h, x = h.contiguous(), x.contiguous()
    e = e.contiguous() if e is not None else None
    params, _ = _params(l)
    tensors = [h, x] + ([e] if e is not None else []) + params
    if not (torch.is_grad_enabled() and any(t.requires_grad for t in tensors)):
        return _forward(l, g, h, x, e, None)
    return _EGNNConvFn.apply(h, x, e, l, g, *params)
