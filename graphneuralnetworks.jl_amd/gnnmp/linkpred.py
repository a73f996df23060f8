"""Link prediction (GraphNeuralNetworks/examples/link_prediction_pubmed.jl): negative_sample and rand_edge_split
(GNNGraphs/src/transform.jl:890-968), DotDecoder (GraphNeuralNetworks/src/layers/basic.jl:210, GNNlib/src/layers/basic.jl:1-3),
WithGraph (basic.jl:40-52) and the adjoint of the per-edge dot product w.r.t. the node features.

Every index and arithmetic step is a libgnnmp call (csrc/linkpred.hip); torch allocates.  The draws are reproducible in `seed` and
are not Julia's RNG stream; `seed=None` takes the next value of a module-level sequence, so a training loop gets fresh negatives on
every call, as the reference does with its global RNG.
"""
from __future__ import annotations

import ctypes
import itertools

import torch

from . import _lib as L
from .graph import GNNGraph, check_num_nodes
from .msgpass import _fused, apply_edges, xi_dot_xj

_MASK64 = (1 << 64) - 1
_seed_counter = itertools.count(1)


def _next_seed() -> int:
    return (0x9E3779B97F4A7C15 * next(_seed_counter)) & _MASK64


def set_seed(seed: int):
    """restart the module-level seed sequence that `seed=None` draws from (Random.seed! for these two transforms)"""
    global _seed_counter
    _seed_counter = itertools.count(1 + (int(seed) & 0xFFFFFFFF) * 1000003)


def negative_sample_prob(num_nodes: int, num_edges: int, num_neg: int) -> float:
    """transform.jl:906-912 in Float64: the sample probability of one trial for `num_neg` codes (already halved when bidirected).
    Positives are the edges plus a self loop on every node.  (Host mirror of the check inside gnnmp_negative_sample.)"""
    maxid = float(num_nodes) * float(num_nodes)
    if maxid == 0.0:
        return 0.0
    pneg = 1.0 - float(num_edges + num_nodes) / (2.0 * maxid)
    if pneg == 0.0:
        return 1.0
    return min(1.0, num_neg / (pneg * maxid) * 1.1)


def negative_sample(g: GNNGraph, num_neg_edges=None, bidirected=None, max_trials: int = 3, seed=None) -> GNNGraph:
    """negative_sample(g; num_neg_edges = g.num_edges, bidirected = is_bidirected(g), max_trials = 3) — transform.jl:890-929: a graph on
    g's nodes whose edges are random non-edges of g (self loops count as edges).  bidirected: num_neg_edges ÷ 2 codes are drawn and
    returned with their reverses.  May hold fewer edges than asked for when the trials run out, as in the reference.  No weights or
    features; g's index dtype and base."""
    assert g.num_graphs == 1
    num = g.num_edges if num_neg_edges is None else int(num_neg_edges)
    if num < 0:
        raise ValueError(f"negative_sample: num_neg_edges = {num} < 0")
    if int(max_trials) < 0:
        raise ValueError(f"negative_sample: max_trials = {max_trials} < 0")
    if bidirected is None:
        from .sampling import is_bidirected
        bidirected = is_bidirected(g)
    bidirected = bool(bidirected)
    half = num // 2 if bidirected else num
    p = negative_sample_prob(g.num_nodes, g.num_edges, half)
    if p < 0.0:       # randsubseq's ArgumentError: more positives than 2 n^2 (multi-edges)
        raise ValueError(f"negative_sample: sample probability {p} < 0 ({g.num_edges} edges on {g.num_nodes} nodes)")
    seed = _next_seed() if seed is None else int(seed) & _MASK64
    cap = 2 * half if bidirected else half
    dt = g.s.dtype
    s_out = torch.empty(max(cap, 1), dtype=dt, device=g.device)
    t_out = torch.empty_like(s_out)
    total = ctypes.c_int64(0)
    L.check(L.load().gnnmp_negative_sample(L.ptr(g.s), L.ptr(g.t), g.idx_bytes, g.index_base, g.num_edges, g.num_nodes, num,
                                           int(bidirected), int(max_trials), ctypes.c_uint64(seed), L.ptr(s_out), L.ptr(t_out), cap,
                                           ctypes.byref(total), L.stream_ptr()))
    k = total.value
    return GNNGraph(s_out[:k], t_out[:k], num_nodes=g.num_nodes, index_base=g.index_base, device=g.device, _validated=True)


def rand_edge_split(g: GNNGraph, frac, bidirected=None, seed=None):
    """rand_edge_split(g, frac; bidirected = is_bidirected(g)) -> g1, g2 — transform.jl:945-968: a uniformly random partition of the
    edges, round(ne frac) of them (half to even) in g1 in permutation order.  bidirected: the edges with s < t are split and each part
    is mirrored, so an edge and its reverse never straddle the split (needs a bidirected graph without self loops or multi-edges:
    IndexError otherwise, the reference's BoundsError).  Both parts keep num_nodes, the index dtype and base; no weights."""
    frac = float(frac)
    if not 0.0 <= frac <= 1.0:
        raise ValueError(f"rand_edge_split: frac = {frac} outside [0, 1]")
    if bidirected is None:
        from .sampling import is_bidirected
        bidirected = is_bidirected(g)
    bidirected = bool(bidirected)
    ne = g.num_edges // 2 if bidirected else g.num_edges
    size1 = int(round(ne * frac))          # Julia's round(Int, x): half to even, as Python's round
    seed = _next_seed() if seed is None else int(seed) & _MASK64
    m = 2 if bidirected else 1
    dt = g.s.dtype
    s1 = torch.empty(m * size1, dtype=dt, device=g.device)
    t1 = torch.empty_like(s1)
    s2 = torch.empty(m * (ne - size1), dtype=dt, device=g.device)
    t2 = torch.empty_like(s2)
    rc = L.load().gnnmp_rand_edge_split(L.ptr(g.s), L.ptr(g.t), g.idx_bytes, g.index_base, g.num_edges, int(bidirected), size1,
                                        ctypes.c_uint64(seed), L.ptr(s1), L.ptr(t1), L.ptr(s2), L.ptr(t2), L.stream_ptr())
    if rc == L.EBOUNDS:
        raise IndexError(L.load().gnnmp_last_error().decode())
    L.check(rc)
    mk = lambda s, t: GNNGraph(s, t, num_nodes=g.num_nodes, index_base=g.index_base, device=g.device, _validated=True)
    return mk(s1, t1), mk(s2, t2)


# ---------------------------------------------------------------------------------------------------------
# the edge decoder and its adjoint
# ---------------------------------------------------------------------------------------------------------
def _use_fused_grad(D: int) -> bool:
    return L.knob(L.KNOB_EDGE_DOT_GRAD) >= 0 and D <= 256


def _compose_grad(g: GNNGraph, xi, xj, dz, alias: bool):
    """the A/B baseline and the D > 256 path: dxi = propagate(w_mul_xj, g, +; xj, w = dz), dxj = the same on the reversed edges
    with xi, alias: dxi + dxj"""
    from .backward import propagate_grad_xj
    dxi = _fused(g, L.W_MUL_XJ, "+", xj, dz)
    dxj = propagate_grad_xj(g, "+", xi, w=dz)
    if not alias:
        return dxi, dxj
    out = torch.empty_like(dxi)
    L.check(L.load().gnnmp_add_f32(L.ptr(dxi), L.ptr(dxj), L.ptr(out), out.numel(), L.stream_ptr()))
    return out, None


def edge_dot_grad(g: GNNGraph, xi, xj, dz, alias: bool = False):
    """The pullback of z = apply_edges(xi_dot_xj, g, xi = xi, xj = xj) ((E, 1)) for dz ((E,) or (E, 1)):
    dxi[v] = Σ_{k: t_k = v} dz_k xj[s_k],  dxj[u] = Σ_{k: s_k = u} dz_k xi[t_k]  -> (dxi, dxj).
    alias = True (xi is xj, DotDecoder): (dxi + dxj, None) from one launch.  Deterministic: no atomics, fixed summation order."""
    check_num_nodes(g, (xi, xj))
    assert xi.dim() == 2 and xj.dim() == 2 and xi.shape == xj.shape and xi.dtype == xj.dtype == torch.float32
    assert not alias or xi is xj
    xi = xi.contiguous()
    xj = xi if alias else xj.contiguous()
    dz = dz.reshape(-1).contiguous().to(torch.float32)
    assert dz.numel() == g.num_edges
    D = xi.shape[1]
    if not _use_fused_grad(D):
        return _compose_grad(g, xi, xj, dz, alias)
    dxi = torch.empty_like(xi)
    dxj = dxi if alias else torch.empty_like(xj)
    rc = L.load().gnnmp_edge_dot_grad_f32(g.plan(False).handle, g.plan_transposed(False).handle, L.ptr(xi), L.ptr(xj), L.ptr(dz),
                                          L.ptr(dxi), L.ptr(dxj), D, L.stream_ptr())
    if rc == L.EUNSUPPORTED:
        return _compose_grad(g, xi, xj, dz, alias)
    L.check(rc)
    return (dxi, None) if alias else (dxi, dxj)


class _EdgeDotFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xi, xj, g):
        ctx.g = g
        ctx.save_for_backward(xi, xj)
        return apply_edges(xi_dot_xj, g, xi=xi, xj=xj)

    @staticmethod
    def backward(ctx, dz):
        xi, xj = ctx.saved_tensors
        dxi, dxj = edge_dot_grad(ctx.g, xi, xj, dz)
        return dxi, dxj, None


class _DotDecoderFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, g):
        ctx.g = g
        ctx.save_for_backward(x)
        return apply_edges(xi_dot_xj, g, xi=x, xj=x)

    @staticmethod
    def backward(ctx, dz):
        (x,) = ctx.saved_tensors
        dx, _ = edge_dot_grad(ctx.g, x, x, dz, alias=True)
        return dx, None


def dot_decoder(g: GNNGraph, x):
    """GNNlib.dot_decoder(g, x) = apply_edges(xi_dot_xj, g, xi = x, xj = x): (E, 1) scores"""
    return apply_edges(xi_dot_xj, g, xi=x, xj=x)


def dot_decoder_ad(g: GNNGraph, x):
    """differentiable dot_decoder: the gradient w.r.t. x is one launch (in-edge and out-edge sums of every node)"""
    check_num_nodes(g, x)
    return _DotDecoderFn.apply(x, g)


def edge_dot_ad(g: GNNGraph, xi, xj):
    """differentiable apply_edges(xi_dot_xj, g, xi = xi, xj = xj): gradients w.r.t. xi and xj"""
    if xi is xj:
        return dot_decoder_ad(g, xi)
    check_num_nodes(g, (xi, xj))
    return _EdgeDotFn.apply(xi, xj, g)


class DotDecoder:
    """DotDecoder() — basic.jl:188-212: for a graph g and node features x, the dot product x_i · x_j on every edge, (E, 1)"""
    takes_graph = True

    def __call__(self, g: GNNGraph, x):
        return dot_decoder(g, x)

    def __repr__(self):
        return "DotDecoder()"


class WithGraph:
    """WithGraph(model, g) — basic.jl:40-52: a model bound to a graph; `m(x)` calls `model(g, x)`, `m(g2, x)` uses g2"""
    takes_graph = True

    def __init__(self, model, g: GNNGraph, traingraph: bool = False):
        self.model, self.g, self.traingraph = model, g, bool(traingraph)

    def __call__(self, *args, **kws):
        if args and isinstance(args[0], GNNGraph):
            return self.model(*args, **kws)
        return self.model(self.g, *args, **kws)

    def __repr__(self):
        return f"WithGraph({self.model!r}, {self.g!r})"
