"""TopKPool and topk_index (GraphNeuralNetworks/src/layers/pool.jl, GNNlib/src/layers/pool.jl:14-27) on csrc/topk.hip:

    y   = p' * X / norm(p)                          gnnmp_topk_score_f32
    idx = topk_index(y, k)                          gnnmp_topk_select_f32 — per member graph of a batch
    A~  = view(A, idx, idx)                         gnnmp_plan_keep_nodes — the child's plan from the parent's, no sort
    X_  = view(X, :, idx) .* σ.(view(y, idx)')      gnnmp_topk_gate_f32; the pullback is gnnmp_topk_gate_grad_f32

The reference's layer holds one dense adjacency matrix.  Here the layer pools a batch: `l(g, x)` returns the child GNNGraph — built as
remove_nodes builds its child, with `.nid` / `.eid` in the parent's numbering — and the gated features.  The reference's topk_index
returns more than k positions when equal values straddle rank k, and its layer then throws; the layer here keeps exactly k per member
graph (equal scores by ascending node id), `topk_index` keeps the reference's "all".  include/gnnmp.h states the order.

torch allocates and slices; every arithmetic step is a libgnnmp call (topk_index turns its keep flags into positions with
torch.nonzero: a compaction, no arithmetic).
"""
from __future__ import annotations

import ctypes
import numbers

import torch

from . import _lib as L
from .graph import GNNGraph, Plan, check_num_edges
from .layers import glorot_uniform
from .transform import _idx_dtype, _node_ptr, _plain_graph, _take

_ACTS = {"sigmoid": L.TOPK_ACT_SIGMOID, "tanh": L.TOPK_ACT_TANH, "identity": L.TOPK_ACT_IDENTITY}
_TIES = {"first": L.TOPK_TIES_FIRST, "all": L.TOPK_TIES_ALL}


def _k_or_ratio(v, who):
    """(k, ratio) of the record: an int is a fixed k >= 1, a float a ratio in (0, 1]"""
    if isinstance(v, bool) or not isinstance(v, numbers.Real):
        raise TypeError(f"{who}: k must be an int (a fixed k) or a float (a ratio), got {type(v).__name__}")
    if isinstance(v, numbers.Integral):
        if v <= 0:
            raise ValueError(f"{who}: k = {v} (k must be at least 1)")
        return int(v), 0.0
    if not 0.0 < float(v) <= 1.0:
        raise ValueError(f"{who}: ratio {v} outside (0, 1]")
    return 0, float(v)


def _f32(t, who, what):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_cuda:
        raise TypeError(f"{who}: {what} must be a float32 tensor on the device")
    return t.contiguous()


def topk_score(x, p):
    """y [N] = x p / norm(p) for x [N, C] (gnnmp_topk_score_f32; norm(p) is computed on the device)"""
    N, C = x.shape
    y = torch.empty(N, dtype=torch.float32, device=x.device)
    L.check(L.load().gnnmp_topk_score_f32(L.ptr(x), L.ptr(p), L.ptr(y), N, C, L.stream_ptr()))
    return y


def topk_select(y, k=0, ratio=0.0, g=None, ties="first", want_rank=False, lds_budget_bytes=0):
    """(keep int32 [N + 1] with keep[N] = 0, rank int32 [N] | None) of gnnmp_topk_select_f32; with a batched g, per member graph"""
    N = y.numel()
    keep = torch.empty(N + 1, dtype=torch.int32, device=y.device)      # (the export's uint32 words: 0 | 1)
    rank = torch.empty(N, dtype=torch.int32, device=y.device) if want_rank else None
    sp = None if g is None else _node_ptr(g)
    job = L.TopkJob(L.ptr(y), L.ptr(sp), 8, g.num_graphs if sp is not None else 1, int(k), float(ratio), _TIES[ties],
                    int(lds_budget_bytes), L.ptr(keep), L.ptr(rank))
    L.check(L.load().gnnmp_topk_select_f32(ctypes.byref(job), N, L.stream_ptr()))
    return keep, rank


def topk_index(y, k, g=None, ties="all"):
    """topk_index(y, k): the positions, ascending and in the index base of node ids (g's; 1 without a graph, as in Julia), of every
    value that is at least the k-th largest — more than k when equal values straddle rank k (ties = "all", the reference's function;
    "first": exactly k, equal values by ascending position).  y: a device vector (or the reference's 1 x N row).  With a batched `g`
    the selection is per member graph and k may also be a ratio in (0, 1]."""
    if ties not in _TIES:
        raise ValueError(f"topk_index: ties {ties!r} (expected 'all' or 'first')")
    k, ratio = _k_or_ratio(k, "topk_index")
    y = _f32(y, "topk_index", "y").reshape(-1)
    base = 1
    if g is not None:
        _plain_graph(g, "topk_index")
        if y.numel() != g.num_nodes:
            raise ValueError(f"topk_index: {y.numel()} values for the {g.num_nodes} nodes of the graph")
        base = g.index_base
    keep, _ = topk_select(y, k, ratio, g, ties)
    idx = torch.nonzero(keep[:-1]).reshape(-1)
    return (idx + base).to(torch.int64 if g is None else _idx_dtype(g))


class TopKPool:
    """TopKPool(k, in_channel) — pool.jl: top-k pooling with the learnable projection `p [in_channel]`.
    k: an int keeps k nodes of every member graph (all of a smaller one), a float in (0, 1] keeps ceil(ratio * n) of each.
    act: "sigmoid" (the reference), "tanh" (Graph U-Net, SAGPool) or "identity".
    The reference's positional form TopKPool(adj, k, in_channel) is accepted with `adj` a GNNGraph, which is then stored: l(x) pools
    it.  A dense adjacency matrix is refused: build the graph with gnnmp.GNNGraph(s, t) and pass that."""

    def __init__(self, *args, act="sigmoid", init=glorot_uniform, seed=None):
        if len(args) == 3:
            adj, k, in_channel = args
            if not isinstance(adj, GNNGraph):
                raise TypeError("TopKPool: a dense adjacency matrix is not supported; pass the graph itself, "
                                "TopKPool(GNNGraph(s, t), k, in_channel), or use TopKPool(k, in_channel) and call l(g, x)")
            _plain_graph(adj, "TopKPool")
            self.g = adj
        elif len(args) == 2:
            k, in_channel = args
            self.g = None
        else:
            raise TypeError("TopKPool(k, in_channel) or TopKPool(g, k, in_channel)")
        self.k, self.ratio = _k_or_ratio(k, "TopKPool")
        if act not in _ACTS:
            raise ValueError(f"TopKPool: act {act!r} (expected 'sigmoid', 'tanh' or 'identity')")
        self.act = act
        self.in_channel = int(in_channel)
        self.p = init(self.in_channel, 1, seed=seed).reshape(-1).contiguous()

    def __call__(self, *args, score=None):
        if len(args) == 1 and self.g is not None:
            return topk_pool(self, self.g, args[0], score=score)
        g, x = args
        return topk_pool(self, g, x, score=score)

    def __repr__(self):
        return f"TopKPool({self.k or self.ratio}, {self.in_channel}, act={self.act})"


def _check(l, g, x, score, who):
    _plain_graph(g, who)
    x = _f32(x, who, "x")
    if x.dim() != 2 or x.shape[0] != g.num_nodes:
        raise ValueError(f"{who}: x has shape {tuple(x.shape)}, expected ({g.num_nodes}, C)")
    if score is None:
        if x.shape[1] != l.in_channel:
            raise ValueError(f"{who}: x has {x.shape[1]} channels, the layer's p has {l.in_channel}")
    else:
        score = _f32(score, who, "score").reshape(-1)
        if score.numel() != g.num_nodes:
            raise ValueError(f"{who}: {score.numel()} scores for the {g.num_nodes} nodes of the graph")
    return x, score


def _plan_keep(pp, g, keep, maps):
    """gnnmp_plan_keep_nodes on one of g's plans -> (child plan, kept nodes, kept edge positions, new id of every parent node)"""
    h = ctypes.c_void_p()
    total = (ctypes.c_int64 * 2)()
    nm = nn = em = None
    if maps:
        nm = torch.empty(pp.n_dst, dtype=torch.int32, device=g.device)
        nn = torch.empty(pp.n_dst, dtype=torch.int32, device=g.device)
        em = torch.empty(pp.n_edges, dtype=torch.int32, device=g.device)
    L.check(L.load().gnnmp_plan_keep_nodes(ctypes.byref(h), pp.handle, L.ptr(keep), L.ptr(nm), L.ptr(nn), L.ptr(em), total, L.stream_ptr()))
    plan = Plan._adopt(h, g.device)
    return (plan, nm[:total[0]], em[:total[1]], nn) if maps else (plan, None, None, None)


def _child(g, keep, edata):
    """the child graph of the keep flags, as remove_nodes builds its own"""
    plan, nid0, eid0, node_new = _plan_keep(g.plan(False), g, keep, True)
    dt = _idx_dtype(g)
    child = GNNGraph._from_plan(plan, g.num_graphs, _take(g.graph_indicator, nid0), _take(g.x, nid0), g.index_base, dt)
    child.w = _take(g.w, eid0)
    child.nid, child.eid = nid0.to(dt) + g.index_base, eid0.to(dt) + g.index_base

    def derive(key):
        pp = g._plans.get(key)
        return None if pp is None else _plan_keep(pp, g, keep, False)[0]
    child._plan_source = derive
    return child, nid0, node_new, (None if edata is None else _take(edata, eid0))


def _gate(x, y, nid0, act):
    out = torch.empty((nid0.numel(), x.shape[1]), dtype=torch.float32, device=x.device)
    job = L.TopkGateJob(L.ptr(x), L.ptr(y), L.ptr(nid0), _ACTS[act], L.ptr(out))
    L.check(L.load().gnnmp_topk_gate_f32(ctypes.byref(job), nid0.numel(), x.shape[1], L.stream_ptr()))
    return out


def _gate_grad(x, y, p, dout, node_new, act, want_dy, want_dp):
    N, C = x.shape
    dx = torch.empty_like(x)
    dy = torch.empty(N, dtype=torch.float32, device=x.device) if want_dy else None
    dp = torch.empty(C, dtype=torch.float32, device=x.device) if want_dp else None
    part = torch.empty(max(1, -(-N // L.TOPK_GRAD_ROWS)) * (C + 1), dtype=torch.float32, device=x.device) if want_dp else None
    job = L.TopkGateGradJob(L.ptr(x), L.ptr(y), L.ptr(p), L.ptr(dout), L.ptr(node_new), _ACTS[act], L.ptr(dx), L.ptr(dy), L.ptr(dp),
                            L.ptr(part))
    L.check(L.load().gnnmp_topk_gate_grad_f32(ctypes.byref(job), N, C, L.stream_ptr()))
    return dx, dy, dp


def _forward(l, g, x, score, edata):
    y = topk_score(x, l.p) if score is None else score
    keep, _ = topk_select(y, l.k, l.ratio, g, "first")
    child, nid0, node_new, e2 = _child(g, keep, edata)
    return child, _gate(x, y, nid0, l.act), y, node_new, e2


def topk_pool(l, g: GNNGraph, x, score=None, edata=None):
    """topk_pool(l, g, x) -> (g2, x2), also l(g, x): the k best-scoring nodes of every member graph of g (y = x p / norm(p), or the given
    `score` [N] — SAGPool, where a conv makes it), the graph they induce and their features gated by act(y).
    g2 is built as remove_nodes builds its child: `.nid` / `.eid` list the kept nodes and edges in g's numbering; the graph indicator,
    the weights and g.x are gathered; num_graphs is kept; the self-looped and transposed plans are derived from g's cached ones with the
    same flags on first use.  With edata -> (g2, x2, edata2).  Heterographs, temporal graphs and sparse-matrix graphs are refused."""
    x, score = _check(l, g, x, score, "topk_pool")
    check_num_edges(g, edata)
    child, x2, _, _, e2 = _forward(l, g, x.detach(), None if score is None else score.detach(), edata)
    return (child, x2) if edata is None else (child, x2, e2)


class _TopKPoolFn(torch.autograd.Function):
    """(x, p | score) -> x2; the child graph leaves through `box` (it carries no gradient)"""

    @staticmethod
    def forward(ctx, x, p_or_score, l, g, given, box):
        child, x2, y, node_new, _ = _forward(l, g, x, p_or_score if given else None, None)
        ctx.save_for_backward(x, y, p_or_score, node_new)
        ctx.act, ctx.given = l.act, given
        box.append(child)
        return x2

    @staticmethod
    def backward(ctx, dout):
        x, y, p_or_score, node_new = ctx.saved_tensors
        want_x, want_2 = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        dout = dout.contiguous()
        if ctx.given:
            dx, dy, _ = _gate_grad(x, y, None, dout, node_new, ctx.act, want_2, False)
            return (dx if want_x else None), dy, None, None, None, None
        dx, _, dp = _gate_grad(x, y, p_or_score, dout, node_new, ctx.act, False, want_2)
        return (dx if want_x else None), dp, None, None, None, None


def topk_pool_ad(l, g: GNNGraph, x, score=None):
    """differentiable topk_pool -> (g2, x2): gradients w.r.t. x and l.p, or w.r.t. x and `score`.  The selection is piecewise constant:
    no gradient flows through it, and g2 carries none.  g2's graph_indicator serves the readouts (global_pool_ad and kin)."""
    x, score = _check(l, g, x, score, "topk_pool_ad")
    box = []
    x2 = _TopKPoolFn.apply(x, l.p if score is None else score, l, g, score is not None, box)
    return box[0], x2
