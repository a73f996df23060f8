"""The transforms that clean up the edge list itself, on the device (csrc/coalesce.hip), and the positional encodings (csrc/rwpe.hip):

  remove_self_loops     GNNGraphs/src/transform.jl:49-64
  remove_edges          GNNGraphs/src/transform.jl:121-146
  remove_multi_edges    GNNGraphs/src/transform.jl:157-185
  to_bidirected         GNNGraphs/src/transform.jl:495-509
  to_unidirected        GNNGraphs/src/transform.jl:517-529
  has_multi_edges       GNNGraphs/src/query.jl:575-579
  has_isolated_nodes    GNNGraphs/src/query.jl:420-422
  random_walk_pe        GNNGraphs/src/transform.jl:975-990

Coalescing parallel edges is a bipartite plan from the input edges to the output edges, and aggregating edge data over it is
propagate(copy_xj, aggr): `coalesce_edges` returns the new graph together with an `EdgeCoalescing` that holds that plan, and the three
reference transforms are thin wrappers.  This container keeps edge data outside the graph (only the weights `g.w` live in it), so every
transform takes `edata` — a tensor [E, ...] or a dict of them — and returns it transformed next to the new graph.

Every index and arithmetic step is a libgnnmp call; torch allocates and slices.
"""
from __future__ import annotations

import ctypes
import numbers

import torch

from . import _lib as L
from .graph import GNNGraph, Plan, check_num_edges
from .msgpass import _flat, _gather, aggr_code

_MODES = {"directed": L.COALESCE_DIRECTED, "mirrored": L.COALESCE_MIRRORED, "undirected": L.COALESCE_UNDIRECTED}
_MASK64 = (1 << 64) - 1


def _like(g: GNNGraph, s, t, w=None) -> GNNGraph:
    """a graph on g's nodes with a new edge list the library produced from g's validated indices"""
    return GNNGraph(s, t, w, num_nodes=g.num_nodes, graph_indicator=g.graph_indicator, num_graphs=g.num_graphs, x=g.x,
                    index_base=g.index_base, device=g.device, _validated=True)


class EdgeCoalescing:
    """The map from the E edges of a graph to the E2 distinct edges of its coalesced form: a plan whose row j lists, in stably sorted
    order, the rows of the original edge data that output edge j collects (a mirrored copy reads the row of the edge it mirrors)."""

    def __init__(self, plan, num_edges_in, num_edges_out):
        self.plan, self.num_edges_in, self.num_edges_out = plan, int(num_edges_in), int(num_edges_out)

    def reduce(self, e, aggr="+"):
        """propagate(copy_xj, aggr) over the plan: e [E] or [E, ...] Float32 -> [E2] or [E2, ...].  Segments of at most the plan's
        split threshold are added in sorted order, bit-identical to the reference's _scatter; `mean` is sum / count."""
        code = aggr_code(aggr)
        assert self.num_edges_in == e.shape[0], f"Got {e.shape[0]} as last dimension size instead of num_edges={self.num_edges_in}"
        ef = _flat(e.reshape(-1, 1) if e.dim() == 1 else e)
        out = torch.empty((self.num_edges_out,) + tuple(e.shape[1:]), dtype=torch.float32, device=e.device)
        if self.num_edges_out == 0:
            return out
        L.check(L.load().gnnmp_propagate_f32(self.plan.handle, L.COPY_XJ, code, L.ptr(ef), None, None, None, L.ptr(out), ef.shape[1],
                                             L.stream_ptr()))
        return out

    def __repr__(self):
        return f"EdgeCoalescing({self.num_edges_in} => {self.num_edges_out})"


def coalesce_edges(g: GNNGraph, mode: str = "directed"):
    """-> (g2, EdgeCoalescing).  mode "directed": the distinct (s, t) pairs of g; "mirrored": those of [s; t], [t; s], which is never
    built; "undirected": the distinct (min(s, t), max(s, t)).  g2's edges ascend lexicographically by (s, t) whether or not g had a
    duplicate; it carries g's nodes, node features, graph indicator, index dtype and base, and no weights."""
    try:
        code = _MODES[mode]
    except (KeyError, TypeError):
        raise ValueError(f"coalesce_edges: mode {mode!r} (expected 'directed', 'mirrored' or 'undirected')")
    E = g.num_edges
    Ev = 2 * E if code == L.COALESCE_MIRRORED else E
    dt = g.s.dtype
    s_out = torch.empty(Ev, dtype=dt, device=g.device)
    t_out = torch.empty(Ev, dtype=dt, device=g.device)
    colptr = torch.empty(Ev + 1, dtype=dt, device=g.device)
    rowval = torch.empty(Ev, dtype=dt, device=g.device)
    job = L.CoalesceJob(L.ptr(g.s), L.ptr(g.t), g.idx_bytes, g.index_base, E, g.num_nodes, code, L.ptr(s_out), L.ptr(t_out),
                        L.ptr(colptr), L.ptr(rowval))
    total = ctypes.c_int64(0)
    L.check(L.load().gnnmp_coalesce_edges(ctypes.byref(job), ctypes.byref(total), L.stream_ptr()))
    k = total.value
    g2 = _like(g, s_out[:k], t_out[:k])
    plan = None
    if k > 0:
        plan = Plan.from_csc(colptr[:k + 1], rowval, n_src=E, n_dst=k, index_base=g.index_base)
    return g2, EdgeCoalescing(plan, E, k)


def _reduce_data(co: EdgeCoalescing, data, aggr):
    if data is None:
        return None
    if isinstance(data, dict):
        return {k: _reduce_data(co, v, aggr) for k, v in data.items()}
    return co.reduce(data, aggr)


def _coalesced(g: GNNGraph, mode, aggr, edata):
    aggr_code(aggr)                      # ValueError before any work
    check_num_edges(g, edata)
    g2, co = coalesce_edges(g, mode)
    g2.w = _reduce_data(co, g.w, aggr)
    return g2 if edata is None else (g2, _reduce_data(co, edata, aggr))


def remove_multi_edges(g: GNNGraph, aggr="+", edata=None):
    """remove_multi_edges(g; aggr = +): parallel edges become one; the weights and `edata` of the copies are combined with `aggr`
    (+, mean, max or min) in the stably sorted order of the edges.  -> g2, or (g2, edata2) when edata is given."""
    return _coalesced(g, "directed", aggr, edata)


def to_bidirected(g: GNNGraph, edata=None):
    """to_bidirected(g): every edge also in the reverse direction, then remove_multi_edges with `mean`, as the reference hard-codes"""
    return _coalesced(g, "mirrored", "mean", edata)


def to_unidirected(g: GNNGraph, edata=None):
    """to_unidirected(g): one edge (min, max) for every connected pair of nodes, data combined with `mean`"""
    return _coalesced(g, "undirected", "mean", edata)


def _compact(g: GNNGraph, rule, edata, remove=None, p=0.0, seed=0):
    check_num_edges(g, edata)
    E = g.num_edges
    dt = g.s.dtype
    s_out = torch.empty(E, dtype=dt, device=g.device)
    t_out = torch.empty(E, dtype=dt, device=g.device)
    eid = torch.empty(E, dtype=dt, device=g.device)
    w_out = None if g.w is None else torch.empty(E, dtype=torch.float32, device=g.device)
    job = L.CompactJob(L.ptr(g.s), L.ptr(g.t), L.ptr(g.w), g.idx_bytes, g.index_base, E, rule, L.ptr(remove),
                       0 if remove is None else remove.numel(), float(p), ctypes.c_uint64(seed), L.ptr(s_out), L.ptr(t_out),
                       L.ptr(w_out), L.ptr(eid))
    total = ctypes.c_int64(0)
    rc = L.load().gnnmp_compact_edges(ctypes.byref(job), ctypes.byref(total), L.stream_ptr())
    if rc == L.EBOUNDS:
        raise IndexError(L.load().gnnmp_last_error().decode())      # the reference's BoundsError
    L.check(rc)
    k = total.value
    g2 = _like(g, s_out[:k], t_out[:k], None if w_out is None else w_out[:k])
    if edata is None:
        return g2
    return g2, _gather(edata, eid[:k], g.index_base)


def remove_self_loops(g: GNNGraph, edata=None):
    """remove_self_loops(g): the edges with s != t, in their order, with their weights and `edata` rows"""
    return _compact(g, L.COMPACT_SELF_LOOPS, edata)


def remove_edges(g: GNNGraph, edges_or_p=0.5, edata=None, seed=None):
    """remove_edges(g, edges_to_remove) / remove_edges(g, p = 0.5): a number is the probability with which every edge is removed
    (reproducible in `seed`; seed = None draws from the module-level sequence of gnnmp.linkpred); an integer sequence or tensor lists
    edge positions in g's index base (repeats allowed; a position outside the edge list is an IndexError)."""
    if isinstance(edges_or_p, numbers.Real) or (isinstance(edges_or_p, torch.Tensor) and edges_or_p.dim() == 0):
        p = float(edges_or_p)
        if not 0.0 <= p <= 1.0:
            raise ValueError(f"remove_edges: probability {p} outside [0, 1]")
        if seed is None:
            from .linkpred import _next_seed
            seed = _next_seed()
        return _compact(g, L.COMPACT_RANDOM, edata, p=p, seed=int(seed) & _MASK64)
    idx = edges_or_p if isinstance(edges_or_p, torch.Tensor) else torch.as_tensor(edges_or_p)
    if idx.dtype.is_floating_point or idx.dtype == torch.bool:
        if idx.numel() > 0:
            raise TypeError("remove_edges: edge positions must be integers")
        idx = idx.to(torch.int64)
    idx = idx.reshape(-1).to(device=g.device, dtype=g.s.dtype).contiguous()
    return _compact(g, L.COMPACT_LIST, edata, remove=idx)


def has_multi_edges(g: GNNGraph) -> bool:
    """has_multi_edges(g): two edges share (s, t)"""
    res = ctypes.c_int(0)
    L.check(L.load().gnnmp_has_multi_edges(L.ptr(g.s), L.ptr(g.t), g.idx_bytes, g.index_base, g.num_edges, ctypes.byref(res),
                                           L.stream_ptr()))
    return bool(res.value)


def has_isolated_nodes(g: GNNGraph, dir: str = "out") -> bool:
    """has_isolated_nodes(g; dir = :out): a node without outgoing (dir = "out") or incoming (dir = "in") edges"""
    if dir not in ("in", "out"):
        raise ValueError(f"has_isolated_nodes: dir {dir!r} (expected 'in' or 'out')")
    plan = g.plan(False) if dir == "in" else g.plan_transposed()
    res = ctypes.c_int(0)
    L.check(L.load().gnnmp_has_isolated_nodes(plan.handle, ctypes.byref(res), L.stream_ptr()))
    return bool(res.value)


def random_walk_pe(g: GNNGraph, walk_length: int):
    """random_walk_pe(g, walk_length): pe[c, k - 1] = (RW^k)[c, c] for k = 1 .. walk_length with RW = A * Diagonal(1 ./ outdegree), A
    the (weighted, when g has weights) adjacency matrix — a Float32 tensor (num_nodes, walk_length), the memory of the reference's
    (walk_length, num_nodes) matrix.  A batched g is walked member by member (block diagonal); nothing N x N is ever formed."""
    if getattr(g, "is_hetero", False) or not isinstance(g, GNNGraph):
        raise TypeError("random_walk_pe: expected a GNNGraph")
    if isinstance(walk_length, bool) or not isinstance(walk_length, numbers.Integral):
        raise TypeError(f"random_walk_pe: walk_length must be an integer, got {type(walk_length).__name__}")
    walk_length = int(walk_length)
    if not 1 <= walk_length <= L.RWPE_MAX_WALK:
        raise ValueError(f"random_walk_pe: walk_length {walk_length} outside 1 .. {L.RWPE_MAX_WALK}")
    out = torch.empty((g.num_nodes, walk_length), dtype=torch.float32, device=g.device)
    if g.num_nodes == 0:
        return out
    sp = None
    if g.num_graphs > 1 and g.graph_indicator is not None:
        # the node offsets of the member graphs: a constant of the batch (gnnmp/utils.py caches the same array)
        sp = g._cache.get("node_ptr")
        if sp is None:
            gi = g.graph_indicator
            sp = torch.empty(g.num_graphs + 1, dtype=torch.int64, device=g.device)
            L.check(L.load().gnnmp_segment_bounds(L.ptr(gi), gi.element_size(), g.index_base, g.num_nodes, g.num_graphs, L.ptr(sp),
                                                  L.stream_ptr()))
            g._cache["node_ptr"] = sp
    job = L.RwpeJob(L.ptr(g.w), L.ptr(sp), 8, g.num_graphs if sp is not None else 1, walk_length, L.ptr(out))
    rc = L.load().gnnmp_random_walk_pe_f32(g.plan_transposed().handle, ctypes.byref(job), L.stream_ptr())
    if rc == L.EINVAL:
        raise ValueError(L.load().gnnmp_last_error().decode())      # an edge between two member graphs, an indicator that is not sorted
    L.check(rc)
    return out
