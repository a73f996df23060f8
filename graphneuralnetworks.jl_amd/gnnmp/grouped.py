"""Grouped dense — one weight per row segment — on csrc/dense_grouped.hip (include/gnnmp.h states the arithmetic):

    out[n] = act(W_g x[n] + b_g)   for the rows n of group g, seg_ptr[g] <= n < seg_ptr[g + 1]       gnnmp_grouped_dense_f32
    dW_g = dz_g' x_g,  db_g = colsum(dz_g)                                                            gnnmp_grouped_dense_grad_w_f32

ONE launch for all groups where a loop of gnnmp.dense spends one a group (two launches for the weight gradient): per-snapshot weights
(EvolveGCNO with grouped=True), per-member-graph or per-node-type linear maps.  seg_ptr stays on the device; torch allocates, every
arithmetic step is a libgnnmp call.  `grouped_launch` / `grouped_grad_launch` take row and group strides for callers that read weights in
place (layers_temporal.evolve_conv); `grouped_dense` and `grouped_dense_ad` are the public forms.
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib as L
from .layers import _ACT

ROUTE_NONE, ROUTE_T16, ROUTE_FMA, ROUTE_GRADW16, ROUTE_GRADW_FMA = 0, 1, 2, 3, 4      # gnnmp_debug_grouped_dense_route's info[0]


def last_route():
    """[kernel, column blocks | slabs, waves, grid.x] of the calling thread's last grouped call (gnnmp_debug_grouped_dense_route)"""
    info = (ctypes.c_int * 4)()
    L.check(L.load().gnnmp_debug_grouped_dense_route(info))
    return list(info)


def seg_ptr_tensor(seg_ptr, device):
    """a device int64 [G + 1] tensor from a tensor or a host list (uploaded once: keep the result to reuse it)"""
    if torch.is_tensor(seg_ptr):
        if seg_ptr.dtype != torch.int64 or seg_ptr.dim() != 1 or seg_ptr.numel() < 1:
            raise TypeError("grouped_dense: seg_ptr must be a one-dimensional int64 tensor of G + 1 row offsets")
        return seg_ptr.to(device).contiguous()
    seg = [int(v) for v in seg_ptr]
    if not seg or seg[0] != 0 or any(b < a for a, b in zip(seg, seg[1:])):
        raise ValueError("grouped_dense: seg_ptr must start at 0 and never decrease")
    return torch.tensor(seg, dtype=torch.int64, device=device)


def grouped_launch(x, ldx, W, w_stride, ldw, w_layout, bias, bias_stride, sp, act, out, ldo, N, G, K, Dout):
    """gnnmp_grouped_dense_f32 on tensors or raw pointers (ctypes.c_void_p): nothing is checked here but by the library"""
    p = lambda v: L.ptr(v) if torch.is_tensor(v) else v      # noqa: E731
    job = L.GroupedDenseJob(p(x), ldx, p(W), w_stride, ldw, int(w_layout), p(bias), bias_stride, p(sp), act, p(out), ldo)
    L.check(L.load().gnnmp_grouped_dense_f32(ctypes.byref(job), N, G, K, Dout, L.stream_ptr()))


def grouped_grad_launch(dz, lddz, x, ldx, sp, dW, dw_stride, db, db_stride, N, G, K, Dout):
    """gnnmp_grouped_dense_grad_w_f32 with a workspace of its own: dW [G][Dout][K] (group stride dw_stride) and / or db"""
    lib = L.load()
    ws = torch.empty(max(1, lib.gnnmp_grouped_dense_grad_workspace(N, G, Dout, K)), dtype=torch.float32, device=dz.device)
    job = L.GroupedDenseGradJob(L.ptr(dz), lddz, L.ptr(x), ldx, L.ptr(sp), L.ptr(dW), dw_stride, L.ptr(db), db_stride, L.ptr(ws), ws.numel())
    L.check(lib.gnnmp_grouped_dense_grad_w_f32(ctypes.byref(job), N, G, K, Dout, L.stream_ptr()))


def _f32(t, what, dims):
    if not torch.is_tensor(t):
        raise TypeError(f"grouped_dense: {what} must be a tensor")
    if t.dtype == torch.float64:
        raise TypeError(f"grouped_dense: Float64 is not supported ({what} is float64); the HIP kernels are Float32")
    if t.dtype != torch.float32 or not t.is_cuda:
        raise TypeError(f"grouped_dense: {what} must be a float32 tensor on the device")
    if t.dim() not in dims:
        raise ValueError(f"grouped_dense: {what} has {t.dim()} dimensions")
    return t


def _rows(t, what):
    """a [N, C] tensor whose rows are contiguous: returned as it is with its row stride (a column block of a panel), else a copy"""
    if t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        t = t.contiguous()
    return t, (t.stride(0) if t.shape[0] > 1 else t.shape[1])


def _checked(x, W, seg_ptr, bias, act, w_layout):
    if w_layout not in (0, 1):
        raise ValueError(f"grouped_dense: w_layout {w_layout!r} (expected 0: W [G, Dout, K], or 1: W [G, K, Dout])")
    if act not in _ACT:
        raise ValueError(f"grouped_dense: act {act!r} (expected None, 'identity' or 'relu')")
    x, W = _f32(x, "x", (2,)), _f32(W, "W", (3,))
    G = W.shape[0]
    Dout, K = (W.shape[1], W.shape[2]) if w_layout == 0 else (W.shape[2], W.shape[1])
    if x.shape[1] != K:
        raise ValueError(f"grouped_dense: x has {x.shape[1]} columns, W contracts over {K}")
    if K < 1 or Dout < 1:
        raise ValueError("grouped_dense: W has an empty dimension")
    sp = seg_ptr_tensor(seg_ptr, x.device)
    if sp.numel() != G + 1:
        raise ValueError(f"grouped_dense: seg_ptr has {sp.numel()} entries for {G} groups (expected {G + 1})")
    if bias is not None:
        bias = _f32(bias, "bias", (1, 2))
        if tuple(bias.shape) not in ((Dout,), (G, Dout)):
            raise ValueError(f"grouped_dense: bias has shape {tuple(bias.shape)}, expected ({Dout},) or ({G}, {Dout})")
        bias = bias.contiguous()
    if W.stride(2) != 1 or W.stride(1) < W.shape[2] or (G > 1 and W.stride(0) < 0):
        W = W.contiguous()
    return x, W, sp, bias, G, K, Dout


def _forward(x, W, sp, bias, code, w_layout, G, K, Dout):
    x, ldx = _rows(x, "x")
    N = x.shape[0]
    out = torch.empty((N, Dout), dtype=torch.float32, device=x.device)
    grouped_launch(x, ldx, W, W.stride(0) if G > 1 else 0, W.stride(1), w_layout, bias, Dout if bias is not None and bias.dim() == 2 else 0,
                   sp, code, out, Dout, N, G, K, Dout)
    return out


def grouped_dense(x, W, seg_ptr, bias=None, act=None, w_layout=0):
    """out [N, Dout]: row n of group g is act(W[g] x[n] + bias[g]).  x [N, K] (a column block of a panel is taken with its row stride);
    W [G, Dout, K], or [G, K, Dout] with w_layout = 1 (row and group strides are taken as they are); bias None, [Dout] (shared) or
    [G, Dout]; seg_ptr the G + 1 row offsets — a device int64 tensor (the caller's contract: non-decreasing from 0 to N), or a host list,
    which is checked and uploaded; act None | 'relu'.  One launch (gnnmp_grouped_dense_f32); empty groups are allowed."""
    x, W, sp, bias, G, K, Dout = _checked(x, W, seg_ptr, bias, act, w_layout)
    return _forward(x.detach(), W.detach(), sp, None if bias is None else bias.detach(), _ACT[act], w_layout, G, K, Dout)


class _GroupedDenseFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, W, bias, sp, code, w_layout, G, K, Dout):
        out = _forward(x, W, sp, bias, code, w_layout, G, K, Dout)
        ctx.save_for_backward(x, W, sp, out if code == L.ACT_RELU else None)
        ctx.v = (code, w_layout, G, K, Dout, None if bias is None else bias.dim())
        return out

    @staticmethod
    def backward(ctx, dy):
        x, W, sp, y = ctx.saved_tensors
        code, w_layout, G, K, Dout, bias_dim = ctx.v
        need_x, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], bias_dim is not None and ctx.needs_input_grad[2]
        dz = dy.contiguous()
        N = dz.shape[0]
        if code == L.ACT_RELU:
            dz2 = torch.empty_like(dz)
            L.check(L.load().gnnmp_act_grad_f32(L.ptr(dz), L.ptr(y), code, L.ptr(dz2), dz.numel(), L.stream_ptr()))
            dz = dz2
        f32 = dict(dtype=torch.float32, device=dz.device)
        dx = dW = db = None
        if need_x:      # dx = dz W_g: the forward with the weight read transposed
            dx = torch.empty((N, K), **f32)
            grouped_launch(dz, Dout, W, W.stride(0) if G > 1 else 0, W.stride(1), 1 - w_layout, None, 0, sp, L.ACT_IDENTITY, dx, K, N, G, Dout, K)
        if need_w or need_b:
            xr, ldx = _rows(x, "x")
            if need_b:
                db = torch.empty((G, Dout) if bias_dim == 2 else (Dout,), **f32)
            if need_w and w_layout == 0:        # dW_g [Dout][K] = dz_g' x_g
                dW = torch.empty((G, Dout, K), **f32)
                grouped_grad_launch(dz, Dout, xr, ldx, sp, dW, Dout * K, db, Dout if bias_dim == 2 else 0, N, G, K, Dout)
            elif need_w:                        # W_g stored [K][Dout]: the operands swapped write that order; db from dz in a call of its own
                dW = torch.empty((G, K, Dout), **f32)
                grouped_grad_launch(xr, ldx, dz, Dout, sp, dW, Dout * K, None, 0, N, G, Dout, K)
                if need_b:
                    grouped_grad_launch(dz, Dout, None, K, sp, None, 0, db, Dout if bias_dim == 2 else 0, N, G, K, Dout)
            else:
                grouped_grad_launch(dz, Dout, None, K, sp, None, 0, db, Dout if bias_dim == 2 else 0, N, G, K, Dout)
        return dx, dW, db, None, None, None, None, None, None


def grouped_dense_ad(x, W, seg_ptr, bias=None, act=None, w_layout=0):
    """differentiable grouped_dense: gradients to x, W and bias (what needs no gradient is not computed) — dx one launch of the forward
    kernel with the weight read transposed, dW and db two launches of gnnmp_grouped_dense_grad_w_f32; no atomics, equal bits run to run."""
    x, W, sp, bias, G, K, Dout = _checked(x, W, seg_ptr, bias, act, w_layout)
    return _GroupedDenseFn.apply(x, W, bias, sp, _ACT[act], w_layout, G, K, Dout)
