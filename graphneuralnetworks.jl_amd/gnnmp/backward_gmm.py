"""GMMConv (MoNet), differentiable: the geometric layer — its edge features are the pseudo-coordinates knn_graph / radius_graph give —
trained on libgnnmp, forward and pullback on the fused mixture-weight kernels.

gmm_conv (GNNlib/src/layers/conv.jl:372-401), edge e: j -> i, kernel k < K, channel c < out (include/gnnmp.h states the arithmetic,
csrc/gmm.hip holds the kernels):

    w_ek = exp(Σ_d ((e_ed − mu_kd)² / 2) sinv_kd²)            [E][K]: one number per edge and kernel       gnnmp_gmm_weights_f32, C = 1
    xk = x dense_x_weight'                                    [N][K out], kernel k's block at k out        gnnmp_dense_f32
    z_ic = (Σ_k (1 / deg_i) Σ_{e into i} w_ek xk[j][k out + c]) / K + bias_c,   y = σ(z) (+ x)             gnnmp_gmm_conv_f32

Neither the [E][K out] weights nor the [N][K out] means of gnnmp.gmm_conv's composition are written.  The pullback mirrors it:

    dz = Δ ⊙ σ'(z)                                                                                         gnnmp_act_grad_z_f32
    dxk [N][K out], dw [E][K]: one walk of the transposed plan                                             gnnmp_gmm_conv_grad_f32
    de [E][ein], dmu, dsigma_inv [K][ein]                                                                  gnnmp_gmm_weights_grad_f32
    d dense_x_weight = dxk' x,  dbias = colsum(dz)                                                         gnnmp_dense_grad_w_f32
    dx = dxk dense_x_weight (+ Δ if the residual was applied)                                              gnnmp_dense_f32, w_layout = 1

torch allocates and slices; every arithmetic step is a libgnnmp call.  What needs_input_grad says is not needed is not computed; z is
kept only when a gradient is needed.  The forward is NOT gnnmp.gmm_conv call for call (it divides by the degree after the row's sum and
folds the kernels in registers): it owes the oracle the 1e-5 bar, not equal bits.  `gnnmp.gmm_conv` / `GMMConv.__call__` are unchanged.
"""
from __future__ import annotations

import ctypes
import warnings

import torch

from . import _lib as L
from .backward import dense_grad_w, dense_grad_x, plan_transposed
from .backward_egnn import act_grad_z
from .graph import GNNGraph, check_num_edges, check_num_nodes
from .layers_more import _ACT_CODES, _add

MAX_K = L.GMM_MAX_K
_RELU_CALLABLES = (torch.relu, torch.nn.functional.relu)


def gmm_weights(e, mu, sigma_inv):
    """w [E][K] of gnnmp_gmm_weights_f32 with C = 1"""
    E, ein = e.shape
    K = mu.shape[0]
    w = torch.empty((E, K), dtype=torch.float32, device=e.device)
    if E > 0:      # (an empty tensor has no address: nothing to launch, nothing to refuse)
        L.check(L.load().gnnmp_gmm_weights_f32(L.ptr(e), L.ptr(mu), L.ptr(sigma_inv), L.ptr(w), E, ein, K, 1, L.stream_ptr()))
    return w


def _p(t):
    """the device pointer, NULL for None and for an empty tensor"""
    return None if t is None or t.numel() == 0 else L.ptr(t)


def gmm_rows(plan, w, xk, bias, act, K, C, want_z):
    """(y [N][C], z [N][C] | None) of gnnmp_gmm_conv_f32"""
    N = xk.shape[0]
    y = torch.empty((N, C), dtype=torch.float32, device=xk.device)
    z = torch.empty_like(y) if want_z else None
    job = L.GmmConvJob(_p(w), _p(xk), _p(bias), _p(y), _p(z), act)
    if N > 0:
        L.check(L.load().gnnmp_gmm_conv_f32(plan.handle, ctypes.byref(job), K, C, L.stream_ptr()))
    return y, z


def gmm_rows_grad(plan, plan_t, w, xk, dz, K, C, want_dxk, want_dw):
    """(dxk [N][K C] | None, dw [E][K] | None) of gnnmp_gmm_conv_grad_f32"""
    dxk = torch.empty_like(xk) if want_dxk else None
    dw = torch.empty_like(w) if want_dw else None
    if want_dw and w.shape[0] == 0:
        if not want_dxk:
            return dxk, dw
        want_dw = False      # no edge: no entry of dw to write
    job = L.GmmConvGradJob(_p(w) if want_dxk else None, _p(xk) if want_dw else None, _p(dz), _p(dxk), _p(dw) if want_dw else None)
    if xk.shape[0] > 0:
        L.check(L.load().gnnmp_gmm_conv_grad_f32(plan.handle, plan_t.handle, ctypes.byref(job), K, C, L.stream_ptr()))
    return dxk, dw


def gmm_weights_grad(e, mu, sigma_inv, w, dw, want_de, want_par):
    """(de [E][ein] | None, dmu, dsigma_inv [K][ein] | None) of gnnmp_gmm_weights_grad_f32; a graph without edges gives zeros"""
    E, ein = e.shape
    K = mu.shape[0]
    de = torch.empty_like(e) if want_de else None
    if E == 0:
        z = (torch.zeros_like(mu), torch.zeros_like(sigma_inv)) if want_par else (None, None)
        return (de, *z)
    dmu = torch.empty_like(mu) if want_par else None
    dsinv = torch.empty_like(sigma_inv) if want_par else None
    part = torch.empty(L.GMM_PARTS * 2 * K * ein, dtype=torch.float32, device=e.device) if want_par else None
    job = L.GmmWeightsGradJob(L.ptr(e), L.ptr(mu), L.ptr(sigma_inv), L.ptr(w), L.ptr(dw), L.ptr(de), L.ptr(dmu), L.ptr(dsinv), L.ptr(part))
    L.check(L.load().gnnmp_gmm_weights_grad_f32(ctypes.byref(job), E, ein, K, L.stream_ptr()))
    return de, dmu, dsinv


def _forward(l, g, x, e, act, want_z):
    """(y before the residual, z | None, w, xk)"""
    from .layers import dense
    K, out = l.K, l.ch[1]
    w = gmm_weights(e, l.mu.contiguous(), l.sigma_inv.contiguous())
    xk = dense(x, l.dense_x_weight)
    bias = None if l.bias is None else l.bias.contiguous()
    y, z = gmm_rows(g.plan(False), w, xk, bias, act, K, out, want_z)
    return y, z, w, xk


class _GMMConvFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, e, mu, sigma_inv, W, bias, l, g, act):
        y, z, w, xk = _forward(l, g, x, e, act, True)
        ctx.residual = l.residual and x.shape[1] == l.ch[1]
        if ctx.residual:
            y = _add(y, x)
        ctx.save_for_backward(x, e, mu, sigma_inv, W, z, w, xk)
        ctx.g, ctx.act, ctx.has_bias, ctx.K, ctx.C = g, act, bias is not None, l.K, l.ch[1]
        return y

    @staticmethod
    def backward(ctx, dy):
        x, e, mu, sigma_inv, W, z, w, xk = ctx.saved_tensors
        g, K, C = ctx.g, ctx.K, ctx.C
        need_x, need_e, need_mu, need_si, need_w = ctx.needs_input_grad[:5]
        need_b = ctx.has_bias and ctx.needs_input_grad[5]
        need_par = need_mu or need_si
        if not (need_x or need_e or need_par or need_w or need_b):
            return (None,) * 9
        dy = dy.contiguous()
        dz = act_grad_z(dy, z, ctx.act)
        dx = de = dmu = dsi = dW = db = None
        want_dxk, want_dw = need_x or need_w, need_e or need_par
        if want_dxk or want_dw:
            dxk, dw = gmm_rows_grad(g.plan(False), plan_transposed(g, False), w, xk, dz, K, C, want_dxk, want_dw)
        if want_dw:
            de, dmu, dsi = gmm_weights_grad(e, mu.contiguous(), sigma_inv.contiguous(), w, dw, need_e, need_par)
            dmu = dmu if need_mu else None
            dsi = dsi if need_si else None
        if need_w:
            dW = dense_grad_w(dxk, x, need_b=False)[0]
        if need_b:
            db = dense_grad_w(dz, x, need_w=False, need_b=True)[1]
        if need_x:
            dx = dense_grad_x(dxk, W)
            if ctx.residual:
                dx = _add(dx, dy)
        return dx, de, dmu, dsi, dW, db, None, None, None


def _act_of(sigma):
    if sigma in _RELU_CALLABLES:
        return L.ACT_RELU
    if callable(sigma):
        raise ValueError(f"gmm_conv_ad: σ = {sigma!r} is a callable; the HIP pullback covers the gnnmp_act names "
                         "(identity, relu, softplus, tanh, swish)")
    if sigma not in _ACT_CODES:
        raise ValueError(f"gmm_conv_ad: activation {sigma!r} is not in the gnnmp_act set (identity, relu, softplus, tanh, swish)")
    return _ACT_CODES[sigma]


def gmm_conv_ad(l, g: GNNGraph, x, e):
    """differentiable GMMConv forward: gradients w.r.t. x, e, l.mu, l.sigma_inv, l.dense_x_weight and l.bias, for σ in the gnnmp_act set
    (identity | relu | softplus | tanh | swish).  Under torch.no_grad(), or when nothing requires a gradient, z is not written."""
    if isinstance(x, (tuple, list)):
        raise NotImplementedError("gmm_conv_ad: a bipartite (xs, xt) input is not covered; pass one feature matrix")
    act = _act_of(l.sigma)
    (nin, ein), out = l.ch
    if l.K > MAX_K:
        raise ValueError(f"gmm_conv_ad: K = {l.K} kernels; 1 .. {MAX_K} are covered (K > {MAX_K} is not)")
    check_num_nodes(g, x)
    check_num_edges(g, e)
    if x.shape[1] != nin:
        raise ValueError(f"gmm_conv_ad: x has {x.shape[1]} features, the layer was built for {nin}")
    if e.dim() != 2 or e.shape[1] != ein:
        raise ValueError(f"gmm_conv_ad: e has {e.shape[-1]} pseudo-coordinates, the layer was built for {ein}")
    if tuple(l.dense_x_weight.shape) != (l.K * out, nin):
        raise ValueError(f"gmm_conv_ad: dense_x_weight is {tuple(l.dense_x_weight.shape)}, (K out, in) = {(l.K * out, nin)} is needed")
    if l.residual and nin != out:
        warnings.warn("Residual not applied : output feature is not equal to input_feature")
    x, e = x.contiguous(), e.contiguous()
    tensors = [x, e, l.mu, l.sigma_inv, l.dense_x_weight] + ([l.bias] if l.bias is not None else [])
    if not (torch.is_grad_enabled() and any(t.requires_grad for t in tensors)):
        y = _forward(l, g, x, e, act, False)[0]
        return _add(y, x) if l.residual and nin == out else y
    return _GMMConvFn.apply(x, e, l.mu, l.sigma_inv, l.dense_x_weight, l.bias, l, g, act)
