"""EvolveGCNO, differentiable (gnnmp/layers_temporal.py; GraphNeuralNetworks/src/layers/temporalconv.jl:678-705): one autograd.Function,
forward and pullback on the batch-one LSTM kernels of csrc/evolve.hip (include/gnnmp.h states their arithmetic).

The forward is evolve_forward call for call — layer(tg, x) and evolve_gcno_ad(layer, tg, x) have equal bits — and keeps the
pre-activations A [T][4D] of the LSTM steps.  The pullback, with M_t = row t of Wseq read as [in][out]:
  the convolutions   over all snapshots at once, at the narrower width: out >= in — Δagg_t = Δy_t M_t' (one gnnmp_dense_f32 a snapshot),
                     Δx = PT(Δagg) (ONE propagate over the transposed batched plan), ΔM_t = agg_t' Δy_t; out < in — Δh = PT(Δy),
                     Δx_t = Δh_t M_t', ΔM_t = x_t' Δh_t.  ΔM_t is gnnmp_dense_grad_w_f32 with the operands swapped (dz = agg_t, x = Δy_t):
                     it then writes [in][out], the flat order of Wseq.  Δb_conv: one column sum.
  the LSTM           T reverse steps: gnnmp_lstm_pointwise_grad_f32 at N = 1 (its record serves unchanged: gx = the kept
                     pre-activations, gh = zeros, b = NULL) gives da_t and Δc_{t-1}; gnnmp_lstm_matvec_grad_f32 with sum = 1 gives
                     Δweight_{t-1} = Wi' da_t + Wh' da_t + ΔM_{t-1} — the step's input and hidden state are one array from step 2
                     on.  Step 1 has them apart: Wi' da_1 is the cotangent of the weight that entered (of conv.weight without a given
                     state), Wh' da_1 that of a given h.
  the LSTM weights   two launches of gnnmp_outer_accum_f32 over all steps: ΔWi = Σ_t da_t x_t', ΔWh = Σ_t da_t h_{t-1}', Δb = Σ_t da_t.
No atomics anywhere; what needs_input_grad rules out is not computed.
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib as L
from .backward import dense_grad_w, propagate_grad_xj
from .layers import gcn_norm_cache
from .layers_temporal import (EvolveGCNOCell, _at, dense_rows, evolve_conv, evolve_inputs, evolve_output, evolve_state, evolve_weights)


def outer_accum(A, B, need_db=False):
    """(dW [R][K], db [R] | None) = (Σ_t A[t] B[t]', Σ_t A[t]) for A [T][R], B [T][K]; T = 0 is the empty sum"""
    T, R = A.shape
    K = B.shape[1]
    f32 = dict(dtype=torch.float32, device=A.device)
    if T == 0:
        return torch.zeros((R, K), **f32), (torch.zeros(R, **f32) if need_db else None)
    A, B = A.contiguous(), B.contiguous()
    dW = torch.empty((R, K), **f32)
    db = torch.empty(R, **f32) if need_db else None
    job = L.OuterAccumJob(L.ptr(A), L.ptr(B), L.ptr(dW), L.ptr(db))
    L.check(L.load().gnnmp_outer_accum_f32(ctypes.byref(job), T, R, K, L.stream_ptr()))
    return dW, db


def lstm_pullback(cell, Wseq, Cseq, A, dM, h0, want_w0=True, want_h0=False, want_c0=False, need_wi=True, need_wh=True, need_b=True):
    """the pullback of evolve_weights: (Δweight_0, Δh_0, Δc_0, ΔWi, ΔWh, Δb) from dM [T] — the cotangents of rows 1 .. T of Wseq, [D] each
    — and what the forward kept (A: the pre-activations).  T reverse steps (one pointwise and one transposed-product call each), then the
    two rank-T updates.  h0: the hidden state that entered, None for zeros (Δh_0 is then None and step 1 adds nothing to ΔWh)."""
    lstm, lib = cell.lstm, L.load()
    T, D = A.shape[0], Wseq.shape[1]
    f32 = dict(dtype=torch.float32, device=A.device)
    want_h0 = want_h0 and h0 is not None
    dA = torch.empty((T, 4 * D), **f32)
    zeros4 = torch.zeros(4 * D, **f32)
    ws = torch.empty(max(1, lib.gnnmp_lstm_matvec_grad_workspace(D)), **f32)
    dh, dc = dM[T - 1], None
    dw0 = dh0 = None
    for t in range(T, 0, -1):
        dcn = torch.empty(D, **f32)
        job = L.LstmGradJob(_at(A, (t - 1) * 4 * D), L.ptr(zeros4), None, _at(Cseq, (t - 1) * D), L.ptr(dh), L.ptr(dc),
                            _at(dA, (t - 1) * 4 * D), L.ptr(dcn))
        L.check(lib.gnnmp_lstm_pointwise_grad_f32(ctypes.byref(job), 1, D, L.stream_ptr()))
        dc = dcn
        da = _at(dA, (t - 1) * 4 * D)
        if t > 1:
            dh = torch.empty(D, **f32)
            job = L.LstmMatvecGradJob(L.ptr(lstm.Wi), L.ptr(lstm.Wh), da, L.ptr(dM[t - 2]), None, L.ptr(dh), None, 1, L.ptr(ws), ws.numel())
            L.check(lib.gnnmp_lstm_matvec_grad_f32(ctypes.byref(job), D, L.stream_ptr()))
        elif want_w0 or want_h0:
            dw0 = torch.empty(D, **f32) if want_w0 else None
            dh0 = torch.empty(D, **f32) if want_h0 else None
            job = L.LstmMatvecGradJob(L.ptr(lstm.Wi), L.ptr(lstm.Wh), da, None, None, L.ptr(dw0), L.ptr(dh0), 0, L.ptr(ws), ws.numel())
            L.check(lib.gnnmp_lstm_matvec_grad_f32(ctypes.byref(job), D, L.stream_ptr()))
    # the LSTM's weights: rank-T updates over all steps
    dWi = dWh = db = None
    if need_wi or need_b:
        dWi, db = outer_accum(dA, Wseq[:T], need_db=need_b)      # the steps' inputs: rows 0 .. T - 1
        if not need_wi:
            dWi = None
    if need_wh:
        if h0 is not None:
            dWh, _ = outer_accum(dA, torch.cat([h0.view(1, D), Wseq[1:T]]))
        else:
            dWh, _ = outer_accum(dA[1:], Wseq[1:T])              # h_0 = 0: step 1 adds nothing
    return dw0, dh0, (dc if want_c0 else None), dWi, dWh, db


class _EvolveFn(torch.autograd.Function):
    """arguments: xcat, w0, h0, c0 (None without a given state), conv.weight, conv.bias, Wi, Wh, b, cell, tg"""

    @staticmethod
    def forward(ctx, xcat, w0, h0, c0, cw, cb, Wi, Wh, b, cell, tg):
        T = tg.num_snapshots
        Wseq, Cseq, A = evolve_weights(cell, T, w0, h0, c0, keep=True)
        y, agg = evolve_conv(cell, tg, xcat, Wseq)
        ctx.cell, ctx.tg, ctx.given = cell, tg, w0 is not None
        ctx.save_for_backward(xcat if agg is None else agg, Wseq, Cseq, A, h0 if h0 is not None else torch.empty(0, device=xcat.device))
        return y

    @staticmethod
    def backward(ctx, dy):
        saved, Wseq, Cseq, A, h0 = ctx.saved_tensors
        cell, tg, given = ctx.cell, ctx.tg, ctx.given
        h0 = h0 if given else None
        need = ctx.needs_input_grad
        cin, out = cell.in_, cell.out
        D, T = cin * out, tg.num_snapshots
        gb, seg = tg.batched()
        lstm = cell.lstm
        f32 = dict(dtype=torch.float32, device=dy.device)
        dy = dy.contiguous()
        c, _, _ = gcn_norm_cache(gb, True)

        def PT(h):
            return propagate_grad_xj(gb, "+", h, scale_src=c, scale_dst=c, add_self_loops=True)

        # ---- the convolutions of all snapshots -------------------------------------------------------------------------------------
        db_conv = dense_grad_w(dy, dy, need_w=False)[1] if (cell.conv.bias is not None and need[5]) else None
        w_first = out < cin
        dz = PT(dy) if w_first else dy                       # the cotangent of the products' outputs
        dx = None
        if need[0]:
            dpre = torch.empty((dy.shape[0], cin), **f32)
            for t in range(T):
                dense_rows(dz, seg[t], seg[t + 1], Wseq[t + 1], cin, out, 0, None, dpre)
            dx = dpre if w_first else PT(dpre)
        dM = []
        for t in range(T):
            r0, r1 = seg[t], seg[t + 1]
            dM.append(dense_grad_w(saved[r0:r1], dz[r0:r1], need_b=False)[0].view(D) if r1 > r0 else torch.zeros(D, **f32))
        want_w0 = need[1] if given else need[4]
        dw0, dh0, dc0, dWi, dWh, db = lstm_pullback(cell, Wseq, Cseq, A, dM, h0, want_w0, given and need[2], given and need[3], need[6], need[7],
                                                    lstm.b is not None and need[8])
        dcw = None
        if not given and dw0 is not None:
            dcw = dw0.view(cin, out).t().contiguous()             # initialstates flattens conv.weight' : back to [out, in]
        return (dx, dw0 if given else None, dh0, dc0, dcw, db_conv, dWi, dWh, db, None, None)


def evolve_gcno_ad(layer, g, x, state=None):
    """differentiable EvolveGCNO / GNNRecurrence(EvolveGCNOCell) / EvolveGCNOCell forward, in the layer's two input forms: a
    TemporalSnapshotsGNNGraph with a list of x_t [N_t, in] -> a list of y_t [N_t, out], or a GNNGraph with x [N, T, in] -> [N, T, out].
    Gradients flow to every x_t, conv.bias, lstm.Wi, lstm.Wh and lstm.b; with state = None also to conv.weight (through initialstates);
    with a state (weight, (h, c)) given to its weight, h and c instead — conv.weight then gets none, exactly as in the reference."""
    name = "evolve_gcno_ad"
    cell = getattr(layer, "cell", layer)
    if not isinstance(cell, EvolveGCNOCell):
        raise TypeError(f"{name}: expected an EvolveGCNOCell or its GNNRecurrence, got {type(cell).__name__}")
    tg, xcat, static = evolve_inputs(name, cell, g, x)
    if not (cell.conv.add_self_loops and not cell.conv.use_edge_weight and cell.conv.sigma is None):
        raise ValueError(f"{name}: the cell's GCNConv must be the reference's (identity σ, self loops, no edge weights)")
    w0, h0, c0 = evolve_state(name, cell, state, xcat.device)
    y = _EvolveFn.apply(xcat, w0, h0, c0, cell.conv.weight, cell.conv.bias, cell.lstm.Wi, cell.lstm.Wh, cell.lstm.b, cell, tg)
    return evolve_output(tg, y, static)
