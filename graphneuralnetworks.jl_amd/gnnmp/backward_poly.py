"""ChebConv and DConv, differentiable: the two polynomial layers trained on libgnnmp, forward and pullback on ONE fused hop kernel.

Both layers run a three-term recurrence over a graph operator (cheb_conv, GNNlib/src/layers/conv.jl:83-98; d_conv, conv.jl:696-724):

    ChebConv   Z_1 = X,  Z_2 = L̃ Z_1,  Z_k = 2 L̃ Z_{k-1} - Z_{k-2},   Y = Σ_k Z_k W_k' .+ b,   L̃ = (2/λ - 1) I - (2/λ) Ã
    DConv      T_1 = S T_0,  T_{i+1} = 2 S T_i - T_0  for S = S_out (over g) and S = S_in (over gᵀ),  S T = A (T .* deg)

gnnmp_poly_hop_f32 (csrc/poly_conv.hip; include/gnnmp.h states the arithmetic) is one order of either in one launch:
out = α (scale_dst .* Σ_slots w ss z[col]) + β self + γ prev + add.  The pullback of such a recurrence is the same recurrence over the
transposed operator with an addend (Clenshaw):

    ChebConv   G_k = ΔY W_k,  B_K = G_K,  B_k = G_k + 2 L̃ᵀ B_{k+1} - B_{k+2}  (k >= 2),  Δx = B_1 = G_1 + L̃ᵀ B_2 - B_3
               L̃ᵀ runs over plan_transposed(g) with its own slot factors: Ã need not be symmetric (the topology is bidirected, the
               weights are whatever the graph carries)
    DConv      per direction C_k = G_k,  C_j = G_j + 2 Sᵀ C_{j+1},  Δx += Sᵀ C_1 - Σ_{j >= 2} C_j;  S_outᵀ is a hop over gᵀ with deg_out as
               scale_dst, S_inᵀ a hop over g with deg_in

so forward and backward cost one launch an order.  dW_k = ΔY' Z_k and db = colsum(ΔY) are the dense adjoints.  The graph's weights and
λmax are constants of the graph, as in the reference.  torch allocates and chains; every arithmetic step is a libgnnmp call.  What
needs_input_grad says is not needed is not computed.

The fused forward rounds differently from gnnmp.cheb_conv / gnnmp.d_conv (one epilogue instead of two or three elementwise passes): the
*_ad functions owe them and the oracle the 1e-5 bar, NOT equal bits.  `gnnmp.cheb_conv` / `gnnmp.d_conv` are unchanged.
Every row is walked whole by one lane group: slow on hub rows.
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib as L
from .backward import dense_grad_w, dense_grad_x, plan_transposed
from .graph import GNNGraph, check_num_nodes, degree
from .layers import dense
from .layers_more import _add, scaled_laplacian_op


def poly_hop(plan, z, alpha, w_slot=None, ss_slot=None, scale_dst=None, beta=0.0, self_=None, gamma=0.0, prev=None, add=None, out=None):
    """out [n_dst][D] of gnnmp_poly_hop_f32; out may be prev or add (then the result replaces it), never z or self_"""
    D = z.shape[1]
    if out is None:
        out = torch.empty((plan.n_dst, D), dtype=torch.float32, device=z.device)
    if plan.n_dst == 0 or D == 0:      # (an empty tensor has no address: nothing to launch, nothing to refuse)
        return out
    job = L.PolyHopJob(L.ptr(z), L.ptr(w_slot), L.ptr(ss_slot), L.ptr(scale_dst), L.ptr(self_), L.ptr(prev), L.ptr(add), float(alpha),
                       float(beta), float(gamma), L.ptr(out))
    L.check(L.load().gnnmp_poly_hop_f32(plan.handle, ctypes.byref(job), D, L.stream_ptr()))
    return out


def _slot_factors(g: GNNGraph, plan, key, node_vec):
    """(ss_slot | None, w_slot | None) of `plan`: node_vec gathered by the slots' sources, the graph's weights by the slots' edges; cached
    on the graph under `key` and the weights' version"""
    key = (key, None if g.w is None else (g.w.data_ptr(), g.w._version))
    hit = g._cache.get(key)
    if hit is None:
        lib = L.load()
        ss = ws = None
        if node_vec is not None:
            ss = torch.empty(plan.n_total, dtype=torch.float32, device=g.device)
            L.check(lib.gnnmp_plan_slot_gather_f32(plan.handle, 0, L.ptr(node_vec), L.ptr(ss), L.stream_ptr()))
        if g.w is not None:
            ws = torch.empty(plan.n_total, dtype=torch.float32, device=g.device)
            L.check(lib.gnnmp_plan_slot_gather_f32(plan.handle, 1, L.ptr(g.w), L.ptr(ws), L.stream_ptr()))
        hit = g._cache[key] = (ss, ws)
    return hit


def _check(name, l_in, g, x):
    if isinstance(x, (tuple, list)):
        raise NotImplementedError(f"{name}: a bipartite (xs, xt) input is not covered; pass one feature matrix")
    if x.dtype != torch.float32:
        raise ValueError(f"{name}: the HIP adjoints are Float32; x is {x.dtype}")
    check_num_nodes(g, x)
    if x.dim() != 2 or x.shape[1] != l_in:
        raise ValueError(f"{name}: x must be [N][{l_in}] for this layer, not {tuple(x.shape)}")


# ---------------------------------------------------------------------------------------------------------
# ChebConv
# ---------------------------------------------------------------------------------------------------------
class _ChebConvFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, g):
        c, ss, ws, lam = scaled_laplacian_op(g)
        plan = g.plan(False)
        K = weight.shape[0]
        a, b = 2.0 / lam, 2.0 / lam - 1.0
        Z = [x]
        if K > 1:
            Z.append(poly_hop(plan, x, -a, ws, ss, c, b, x))
        for _ in range(2, K):
            Z.append(poly_hop(plan, Z[-1], -2.0 * a, ws, ss, c, 2.0 * b, Z[-1], -1.0, Z[-2]))
        Y = dense(Z[0], weight[0])
        for k in range(1, K):
            Y = _add(Y, dense(Z[k], weight[k]))
        if bias is not None:
            from .layers import bias_act
            Y = bias_act(Y, bias, None)
        need_w = ctx.needs_input_grad[1]
        ctx.save_for_backward(weight, *(Z if need_w else ()))      # the Z_k are kept for dW_k only: Δx needs none of them
        ctx.g, ctx.lam, ctx.has_bias = g, lam, bias is not None
        return Y

    @staticmethod
    def backward(ctx, dY):
        weight, *Z = ctx.saved_tensors
        g, lam = ctx.g, ctx.lam
        K = weight.shape[0]
        need_x, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        need_b = ctx.has_bias and ctx.needs_input_grad[2]
        dY = dY.contiguous()
        dx = dW = db = None
        if need_w:
            per = []
            for k in range(K):
                dWk, dbk = dense_grad_w(dY, Z[k], need_b=need_b and k == 0)
                per.append(dWk)
                db = dbk if k == 0 else db
            dW = torch.stack(per)                                   # a copy, no arithmetic
        elif need_b:
            db = dense_grad_w(dY, dY, need_w=False)[1]
        if need_x:
            c = scaled_laplacian_op(g)[0]
            pt = plan_transposed(g, False)
            sst, wst = _slot_factors(g, pt, "cheb_t", c)            # Ãᵀ: row j lists the edges that leave j, its sources are their targets
            a, b = 2.0 / lam, 2.0 / lam - 1.0
            B1 = B2 = None                                          # B_{k+1}, B_{k+2}
            for k in range(K, 0, -1):
                G = dense_grad_x(dY, weight[k - 1])
                if B1 is None:
                    Bk = G
                elif k >= 2:
                    Bk = poly_hop(pt, B1, -2.0 * a, wst, sst, c, 2.0 * b, B1, -1.0 if B2 is not None else 0.0, B2, G, out=G)
                else:
                    Bk = poly_hop(pt, B1, -a, wst, sst, c, b, B1, -1.0 if B2 is not None else 0.0, B2, G, out=G)
                B1, B2 = Bk, B1
            dx = B1
        return dx, dW, db, None


def cheb_conv_ad(l, g: GNNGraph, x):
    """differentiable ChebConv forward: gradients w.r.t. x, l.weight and l.bias; k = 1, 2, ... — one gnnmp_poly_hop_f32 launch an order in
    either direction.  Within 1e-5 of gnnmp.cheb_conv, not bit for bit (the recurrence's three terms are one epilogue here)."""
    _check("cheb_conv_ad", l.weight.shape[2], g, x)
    return _ChebConvFn.apply(x.contiguous(), l.weight, l.bias, g)


# ---------------------------------------------------------------------------------------------------------
# DConv
# ---------------------------------------------------------------------------------------------------------
def _dconv_ops(g: GNNGraph):
    """per direction d (0: the steps over gᵀ that feed weights[0], 1: the steps over g that feed weights[1]) the forward hop's
    (plan, w_slot, ss_slot) and the adjoint's (plan, w_slot, scale_dst): the degree factors in slot order, once per graph"""
    deg_out, deg_in = degree(g, torch.float32, dir="out"), degree(g, torch.float32, dir="in")
    fplan, bplan = g.plan(False), plan_transposed(g, False)
    ss_f, ws_f = _slot_factors(g, fplan, "dconv_f", deg_out)
    ss_b, ws_b = _slot_factors(g, bplan, "dconv_b", deg_in)
    fwd = ((bplan, ws_b, ss_b), (fplan, ws_f, ss_f))
    adj = ((fplan, ws_f, deg_in), (bplan, ws_b, deg_out))
    return fwd, adj


def _dconv_slices(k):
    """the weight slice each term T_0 .. T_k of a direction multiplies, as the reference wrote it: T_0 slice 0, T_1 slice 1, and the loop
    `for i in 2:k` reads slice i for T_i's successor — slice 1 (0-based) twice"""
    return [0] if k == 1 else [0, 1] + list(range(1, k))


class _DConvFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weights, bias, g):
        k = weights.shape[1]
        fwd, _ = _dconv_ops(g)
        idx = _dconv_slices(k)
        T = [[x], [x]]                                              # T[d][j]; T_0 is never advanced
        for d in (0, 1):
            plan, ws, ss = fwd[d]
            if k > 1:
                T[d].append(poly_hop(plan, x, 1.0, ws, ss))
            for _ in range(1, k):
                T[d].append(poly_hop(plan, T[d][-1], 2.0, ws, ss, gamma=-1.0, prev=x))
        h = None
        for j, i in enumerate(idx):
            term = dense(T[0][j], weights[0, i], None, None, x2=T[1][j], W2=weights[1, i])
            h = term if h is None else _add(h, term)
        if bias is not None:
            from .layers import bias_act
            h = bias_act(h, bias, None)
        need_w = ctx.needs_input_grad[1]
        ctx.save_for_backward(weights, *((T[0] + T[1]) if need_w else ()))
        ctx.g, ctx.has_bias = g, bias is not None
        return h

    @staticmethod
    def backward(ctx, dY):
        weights, *Ts = ctx.saved_tensors
        g = ctx.g
        k = weights.shape[1]
        idx = _dconv_slices(k)
        n = len(idx)
        need_x, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        need_b = ctx.has_bias and ctx.needs_input_grad[2]
        dY = dY.contiguous()
        dx = dW = db = None
        if need_w:
            T = (Ts[:n], Ts[n:])
            rows = []
            for d in (0, 1):
                per = [None] * k
                for j, i in enumerate(idx):
                    dWj, dbj = dense_grad_w(dY, T[d][j], need_b=need_b and d == 0 and j == 0)
                    per[i] = dWj if per[i] is None else _add(per[i], dWj)      # slice 1 collects two terms
                    db = dbj if (d == 0 and j == 0) else db
                rows.append(torch.stack(per))
            dW = torch.stack(rows)
        elif need_b:
            db = dense_grad_w(dY, dY, need_w=False)[1]
        if need_x:
            _, adj = _dconv_ops(g)
            dx = _add(dense_grad_x(dY, weights[0, 0]), dense_grad_x(dY, weights[1, 0]))
            for d in (0, 1):
                if n == 1:
                    break
                plan, ws, sd = adj[d]
                C = dense_grad_x(dY, weights[d, idx[n - 1]])        # C_k
                R = None                                            # Σ_{j >= 2} C_j: what the `- T_0` terms send to x
                for j in range(n - 2, 0, -1):
                    R = C if R is None else _add(R, C)
                    G = dense_grad_x(dY, weights[d, idx[j]])
                    C = poly_hop(plan, C, 2.0, ws, None, sd, add=G, out=G)
                # Δx += Sᵀ C_1 - R, accumulated through add
                dx = poly_hop(plan, C, 1.0, ws, None, sd, gamma=-1.0 if R is not None else 0.0, prev=R, add=dx, out=dx)
        return dx, dW, db, None


def d_conv_ad(l, g: GNNGraph, x):
    """differentiable DConv forward: gradients w.r.t. x, l.weights and l.bias.  The forward is gnnmp.d_conv's with every `2 * step - T0` as
    one hop (within 1e-5 of it, not bit for bit); the backward follows the forward as the reference wrote it — T0 is never advanced and
    weight slice 2 (1-based) is read twice."""
    _check("d_conv_ad", l.weights.shape[3], g, x)
    return _DConvFn.apply(x.contiguous(), l.weights, l.bias, g)
