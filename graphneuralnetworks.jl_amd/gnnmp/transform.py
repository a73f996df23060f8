"""The transforms that clean up the edge list itself, on the device (csrc/coalesce.hip), and the positional encodings (csrc/rwpe.hip):

  remove_self_loops     GNNGraphs/src/transform.jl:49-64
  remove_edges          GNNGraphs/src/transform.jl:121-146
  remove_multi_edges    GNNGraphs/src/transform.jl:157-185
  to_bidirected         GNNGraphs/src/transform.jl:495-509
  to_unidirected        GNNGraphs/src/transform.jl:517-529
  has_multi_edges       GNNGraphs/src/query.jl:575-579
  has_isolated_nodes    GNNGraphs/src/query.jl:420-422
  random_walk_pe        GNNGraphs/src/transform.jl:975-990
  ppr_diffusion         GNNGraphs/src/transform.jl:1026-1051   (csrc/ppr.hip)
  remove_nodes          GNNGraphs/src/transform.jl:212-276
  add_edges             GNNGraphs/src/transform.jl:319-353
  perturb_edges         GNNGraphs/src/transform.jl:385-420
  add_nodes             GNNGraphs/src/transform.jl:553-561

Coalescing parallel edges is a bipartite plan from the input edges to the output edges, and aggregating edge data over it is
propagate(copy_xj, aggr): `coalesce_edges` returns the new graph together with an `EdgeCoalescing` that holds that plan, and the three
reference transforms are thin wrappers.  This container keeps edge data outside the graph (only the weights `g.w` live in it), so every
transform takes `edata` — a tensor [E, ...] or a dict of them — and returns it transformed next to the new graph.

The four structural augmentations at the end of the list edit the graph's PLAN (csrc/plan_edit.hip): the child's dst-sorted CSR is
written from the parent's cached plan without a sort, once per kind of plan the parent holds (plain, self-looped, transposed), lazily.

Every index and arithmetic step is a libgnnmp call; torch allocates and slices.
"""
from __future__ import annotations

import ctypes
import math
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
    sp = _node_ptr(g)
    job = L.RwpeJob(L.ptr(g.w), L.ptr(sp), 8, g.num_graphs if sp is not None else 1, walk_length, L.ptr(out))
    rc = L.load().gnnmp_random_walk_pe_f32(g.plan_transposed().handle, ctypes.byref(job), L.stream_ptr())
    if rc == L.EINVAL:
        raise ValueError(L.load().gnnmp_last_error().decode())      # an edge between two member graphs, an indicator that is not sorted
    L.check(rc)
    return out


def _node_ptr(g: GNNGraph):
    """the node offsets of the member graphs of a batch (None for one graph): a constant of the batch (gnnmp/utils.py caches the same
    array)"""
    if not (g.num_graphs > 1 and g.graph_indicator is not None):
        return None
    sp = g._cache.get("node_ptr")
    if sp is None:
        gi = g.graph_indicator
        sp = torch.empty(g.num_graphs + 1, dtype=torch.int64, device=g.device)
        L.check(L.load().gnnmp_segment_bounds(L.ptr(gi), gi.element_size(), g.index_base, g.num_nodes, g.num_graphs, L.ptr(sp),
                                              L.stream_ptr()))
        g._cache["node_ptr"] = sp
    return sp


def ppr_diffusion(g: GNNGraph, alpha=0.85, *, lds_budget_bytes: int = 160 * 1024) -> GNNGraph:
    """ppr_diffusion(g; alpha = 0.85f0): g with the weight of every edge s -> t replaced by alpha * inv(I + (alpha - 1) * A)[t, s], A the
    (weighted, when g has weights; parallel edges summed) adjacency matrix with A[t, s] for the edge s -> t — what the reference's CODE
    computes (its docstring speaks of a column normalisation that the code does not do).  Float32, alpha rounded to float32 once.  Only
    existing edges are re-weighted; every copy of a multi-edge receives the same value; a graph without weights comes back weighted.
    A batched g is inverted member by member on the device (block diagonal; csrc/ppr.hip): nothing N x N is formed unless g is one
    graph, and a member graph may have at most PPR_MAX_NODES nodes.  A singular I + (alpha - 1) * A is a ValueError (the reference's
    SingularException), as are an edge between two member graphs and an unsorted graph_indicator.  Not differentiable.
    The result shares g's nodes, features, indicator and plans, as set_edge_weight's does.
    lds_budget_bytes (keyword only): the record's field of that name, passed through as it is — a tuning knob, the result does not
    depend on it.  The mirror asks for the largest, 160 KB, which keeps member graphs of up to 201 nodes in LDS (a launch takes only what its largest such graph needs, so a
    batch of small graphs pays nothing for it; measured, DESIGN.md §5: a batch of 150-node graphs is about 300 times faster than at the
    record's own default, 0 = 64 KB = 127 nodes, which sends them through device scratch one after another)."""
    _plain_graph(g, "ppr_diffusion")
    if isinstance(alpha, bool) or not isinstance(alpha, numbers.Real):
        raise TypeError(f"ppr_diffusion: alpha must be a real number, got {type(alpha).__name__}")
    alpha = float(alpha)
    if not math.isfinite(alpha):
        raise ValueError(f"ppr_diffusion: alpha {alpha} is not finite")
    out = torch.empty(g.num_edges, dtype=torch.float32, device=g.device)
    if g.num_nodes > 0 and g.num_edges > 0:
        sp = _node_ptr(g)
        job = L.PprJob(L.ptr(g.w), L.ptr(sp), 8, g.num_graphs if sp is not None else 1, alpha, int(lds_budget_bytes), L.ptr(out))
        rc = L.load().gnnmp_ppr_diffusion_f32(g.plan_transposed().handle, ctypes.byref(job), L.stream_ptr())
        if rc == L.EINVAL:
            raise ValueError(L.load().gnnmp_last_error().decode())      # a singular block, an edge between two member graphs, ...
        L.check(rc)
    g2 = GNNGraph(g.s, g.t, out, num_nodes=g.num_nodes, graph_indicator=g.graph_indicator, num_graphs=g.num_graphs, x=g.x,
                  index_base=g.index_base, device=g.device, _validated=True)
    g2._plans = g._plans      # same (s, t): the plans are shared, as set_edge_weight shares them
    if "node_ptr" in g._cache:
        g2._cache["node_ptr"] = g._cache["node_ptr"]      # same nodes and indicator: a second diffusion or random_walk_pe reuses the offsets
    return g2


# ---------------------------------------------------------------------------------------------------------
# structural augmentations on derived plans (csrc/plan_edit.hip)
# ---------------------------------------------------------------------------------------------------------
def _plain_graph(g, who):
    """the four augmentations take a COO GNNGraph; the other containers are refused by name"""
    if getattr(g, "is_hetero", False):
        raise TypeError(f"{who}: GNNHeteroGraph is not supported")
    from .temporal_graph import TemporalSnapshotsGNNGraph
    if isinstance(g, TemporalSnapshotsGNNGraph):
        raise TypeError(f"{who}: TemporalSnapshotsGNNGraph is not supported")
    if not isinstance(g, GNNGraph):
        raise TypeError(f"{who}: expected a GNNGraph, got {type(g).__name__}")
    if g.graph_type == "sparse":
        raise TypeError(f"{who}: sparse-matrix graphs (GNNGraph.from_sparse) are not supported")


def _idx_dtype(g: GNNGraph):
    return torch.int64 if g.idx_bytes == 8 else torch.int32


def _take(x, idx0):
    """rows idx0 (int32, 0-based) of a feature tensor / dict of them; index vectors are copied word by word through the float gather"""
    if x is None:
        return None
    if isinstance(x, dict):
        return {k: _take(v, idx0) for k, v in x.items()}
    if idx0.numel() == 0:
        return x[:0].clone()
    if x.dtype in (torch.int64, torch.int32):
        words = 2 if x.dtype == torch.int64 else 1
        src = x.contiguous().view(torch.float32).view(x.shape[0], words)
        return _gather(src, idx0, 0).view(x.dtype).view(idx0.numel())
    return _gather(x, idx0, 0)


def _cat(a, b):
    if isinstance(a, dict):
        if not isinstance(b, dict) or sorted(a) != sorted(b):
            raise ValueError("cannot concatenate feature data with different keys")
        return {k: _cat(a[k], b[k]) for k in a}
    return torch.cat([a, torch.as_tensor(b).to(device=a.device, dtype=a.dtype)])


def _seed64(seed):
    if seed is None:
        from .linkpred import _next_seed
        seed = _next_seed()
    return int(seed) & _MASK64


def _plan_remove(pp: Plan, g: GNNGraph, lst, p, seed, maps):
    """gnnmp_plan_remove_nodes on one of g's plans -> (child plan, kept nodes, kept edge positions): int32, 0-based, None unless `maps`"""
    h = ctypes.c_void_p()
    total = (ctypes.c_int64 * 2)()
    nm = em = None
    if maps:
        nm = torch.empty(pp.n_dst, dtype=torch.int32, device=g.device)
        em = torch.empty(pp.n_edges, dtype=torch.int32, device=g.device)
    rc = L.load().gnnmp_plan_remove_nodes(ctypes.byref(h), pp.handle, L.ptr(lst), g.idx_bytes, g.index_base,
                                          0 if lst is None else lst.numel(), float(p), ctypes.c_uint64(seed), L.ptr(nm), None, L.ptr(em),
                                          total, L.stream_ptr())
    if rc == L.EBOUNDS:
        raise IndexError(L.load().gnnmp_last_error().decode())
    L.check(rc)
    plan = Plan._adopt(h, g.device)
    return (plan, nm[:total[0]], em[:total[1]]) if maps else (plan, None, None)


def remove_nodes(g: GNNGraph, nodes_or_p, edata=None, seed=None):
    """remove_nodes(g, nodes_to_remove) / remove_nodes(g, p): the graph without the listed nodes (ids in g's index base, any order,
    repeats allowed; an id outside the graph is an IndexError) or without the nodes a Bernoulli(p) mask drops (reproducible in `seed`;
    seed = None draws from the module-level sequence of gnnmp.linkpred), and without every edge that touched one.  The kept nodes and
    edges keep their order and are renumbered; `.nid` / `.eid` of the result list them in g's numbering, as induced_subgraph sets them.
    Node features, weights and `edata` follow.  -> g2, or (g2, edata2) when edata is given.

    Deviation: the reference passes g's graph_indicator through unchanged (then longer than the new node count); here it is gathered by
    `.nid`, and num_graphs is kept.

    g2's plans are derived from g's cached plans of the same kind (gnnmp_plan_remove_nodes: no sort), each on first use."""
    _plain_graph(g, "remove_nodes")
    check_num_edges(g, edata)
    lst, p = None, 0.0
    if isinstance(nodes_or_p, numbers.Real) and not isinstance(nodes_or_p, numbers.Integral) or (
            isinstance(nodes_or_p, torch.Tensor) and nodes_or_p.dim() == 0 and nodes_or_p.dtype.is_floating_point):
        p = float(nodes_or_p)
        if not 0.0 <= p <= 1.0:
            raise ValueError(f"remove_nodes: probability {p} outside [0, 1]")
        seed = _seed64(seed)
    else:
        idx = nodes_or_p if isinstance(nodes_or_p, torch.Tensor) else torch.as_tensor(nodes_or_p)
        if idx.dtype.is_floating_point or idx.dtype == torch.bool:
            if idx.numel() > 0:
                raise TypeError("remove_nodes: node ids must be integers")
            idx = idx.to(torch.int64)
        lst = idx.reshape(-1).to(device=g.device, dtype=_idx_dtype(g)).contiguous()
        seed = 0
    plan, nid0, eid0 = _plan_remove(g.plan(False), g, lst, p, seed, True)
    dt = _idx_dtype(g)
    child = GNNGraph._from_plan(plan, g.num_graphs, _take(g.graph_indicator, nid0), _take(g.x, nid0), g.index_base, dt)
    child.w = _take(g.w, eid0)
    child.nid, child.eid = nid0.to(dt) + g.index_base, eid0.to(dt) + g.index_base

    def derive(key):
        pp = g._plans.get(key)
        return None if pp is None else _plan_remove(pp, g, lst, p, seed, False)[0]
    child._plan_source = derive
    return child if edata is None else (child, _take(edata, eid0))


def _plan_add(pp: Plan, g: GNNGraph, s_new, t_new, m, n_nodes, seed=0, outs=(None, None)):
    h = ctypes.c_void_p()
    rc = L.load().gnnmp_plan_add_edges(ctypes.byref(h), pp.handle, L.ptr(s_new), L.ptr(t_new), g.idx_bytes, g.index_base, m, n_nodes,
                                       ctypes.c_uint64(seed), L.ptr(outs[0]), L.ptr(outs[1]), L.stream_ptr())
    if rc == L.EBOUNDS:
        raise AssertionError(L.load().gnnmp_last_error().decode())      # the reference's @assert minimum(snew) >= 1
    L.check(rc)
    return Plan._adopt(h, g.device)


def _grow(g: GNNGraph, s_new, t_new, w_new, m, n_nodes, x_new=None, gi_new=None, seed=None):
    """g plus m edges (s_new = None: drawn on the device from `seed`) on n_nodes >= g.num_nodes nodes"""
    N = g.num_nodes
    x, gi = g.x, g.graph_indicator
    if n_nodes > N:
        if (x is None) != (x_new is None):
            raise ValueError("node features for the new nodes are needed exactly when the graph has node features"
                             f" ({n_nodes - N} new nodes)")
        if x is not None:
            x_new = torch.as_tensor(x_new).to(device=g.device, dtype=torch.float32)
            if x_new.shape[0] != n_nodes - N or tuple(x_new.shape[1:]) != tuple(x.shape[1:]):
                raise ValueError(f"expected node features of shape {(n_nodes - N,) + tuple(x.shape[1:])}, got {tuple(x_new.shape)}")
            x = torch.cat([x, x_new])
        if gi is not None:
            if gi_new is None:
                raise ValueError("new nodes of a batched graph need their graph_indicator (add_nodes(g, n, graph_indicator = ...))")
            gi_new = torch.as_tensor(gi_new).reshape(-1).to(device=g.device, dtype=gi.dtype)
            if gi_new.numel() != n_nodes - N:
                raise ValueError(f"expected {n_nodes - N} graph_indicator entries, got {gi_new.numel()}")
            gi = torch.cat([gi, gi_new])
    dt = _idx_dtype(g)
    if s_new is None and m > 0:
        s_new, t_new = torch.empty(m, dtype=dt, device=g.device), torch.empty(m, dtype=dt, device=g.device)
        plan = _plan_add(g.plan(False), g, None, None, m, n_nodes, seed, (s_new, t_new))
    else:
        plan = _plan_add(g.plan(False), g, s_new, t_new, m, n_nodes)
    child = GNNGraph._from_plan(plan, g.num_graphs, gi, x, g.index_base, dt)
    if g.w is not None or w_new is not None:                       # cat_features (utils.jl:119-122): a missing side is ones
        w_old = g.w if g.w is not None else torch.ones(g.num_edges, dtype=torch.float32, device=g.device)
        child.w = torch.cat([w_old, w_new if w_new is not None else torch.ones(m, dtype=torch.float32, device=g.device)])

    def derive(key):
        pp = g._plans.get(key)
        if pp is None:
            return None
        return _plan_add(pp, g, t_new, s_new, m, n_nodes) if isinstance(key, tuple) else _plan_add(pp, g, s_new, t_new, m, n_nodes)
    child._plan_source = derive
    return child


def add_edges(g: GNNGraph, s, t=None, w=None, edata=None, new_edata=None, num_nodes=None):
    """add_edges(g, s, t) / add_edges(g, (s, t)) / add_edges(g, (s, t, w)): g with the edges s -> t appended to its edge list.  Weights
    follow the reference's cat_features: when only one side has them the other side weighs 1.  `edata` (g's) and `new_edata` (the new
    edges') are concatenated and returned next to the graph.  No new edge returns g itself.  An index above g.num_nodes adds nodes
    (num_nodes = ... says how many the result has and saves reading the maximum back); they need rows of node features when g has
    them, which add_nodes takes — here that is a ValueError.  An index below the index base is an AssertionError, as in the reference.

    The result's plans are derived from g's cached plans of the same kind (gnnmp_plan_add_edges), each on first use."""
    _plain_graph(g, "add_edges")
    if t is None and isinstance(s, (tuple, list)) and len(s) in (2, 3) and not isinstance(s[0], numbers.Number):
        tup = s
        s, t = tup[0], tup[1]
        w = tup[2] if len(tup) == 3 else w
    if t is None:
        raise TypeError("add_edges: expected (g, s, t), (g, (s, t)) or (g, (s, t, w))")
    check_num_edges(g, edata)
    dt = _idx_dtype(g)
    s = torch.as_tensor(s).reshape(-1).to(device=g.device, dtype=dt).contiguous()
    t = torch.as_tensor(t).reshape(-1).to(device=g.device, dtype=dt).contiguous()
    assert s.numel() == t.numel(), "length(snew) == length(tnew)"
    m = s.numel()
    if w is not None:
        w = torch.as_tensor(w).reshape(-1).to(device=g.device, dtype=torch.float32).contiguous()
        assert w.numel() == m, "length(wnew) == length(snew)"
    if m == 0:
        return g if edata is None else (g, edata)
    if (edata is None) != (new_edata is None):
        raise ValueError("add_edges: edata and new_edata go together")
    if num_nodes is None:
        n_nodes = max(g.num_nodes, int(torch.maximum(s.max(), t.max())) + 1 - g.index_base)
    else:
        n_nodes = int(num_nodes)
        if n_nodes < g.num_nodes:
            raise ValueError(f"add_edges: num_nodes = {n_nodes} below the graph's {g.num_nodes} nodes")
    if n_nodes > g.num_nodes and g.x is not None:
        raise ValueError(f"add_edges: {n_nodes - g.num_nodes} new nodes without node features (add_nodes(g, n, x) first)")
    child = _grow(g, s, t, w, m, n_nodes)
    return child if edata is None else (child, _cat(edata, new_edata))


def add_nodes(g: GNNGraph, n: int, x=None, graph_indicator=None):
    """add_nodes(g, n; ndata): n new, isolated nodes g.num_nodes + 1 .. g.num_nodes + n.  `x` [n, ...] is required exactly when g has
    node features; a batched g also needs the new nodes' graph_indicator (in g's index base)."""
    _plain_graph(g, "add_nodes")
    if isinstance(n, bool) or not isinstance(n, numbers.Integral) or n < 0:
        raise ValueError(f"add_nodes: n must be a non-negative integer, got {n!r}")
    if n == 0:
        if x is not None and torch.as_tensor(x).shape[0] != 0:
            raise ValueError("add_nodes: node features for 0 new nodes")
        return g
    return _grow(g, None, None, None, 0, g.num_nodes + int(n), x_new=x, gi_new=graph_indicator)


def perturb_edges(g: GNNGraph, perturb_ratio, seed=None):
    """perturb_edges(g, perturb_ratio): g plus ceil(num_edges * perturb_ratio) random edges without self loops, uniform over the ordered
    pairs of distinct nodes (the distribution of the reference's rejection loop; the draw is the library's hash, reproducible in
    `seed`; seed = None draws from the module-level sequence of gnnmp.linkpred).  The new edges of a weighted graph weigh 1."""
    _plain_graph(g, "perturb_edges")
    assert 0 <= perturb_ratio <= 1, "perturb_ratio must be between 0 and 1"
    m = math.ceil(g.num_edges * float(perturb_ratio))
    if m == 0:
        return g
    assert g.num_nodes > 1, "Graph must contain at least 2 nodes to add edges"
    return _grow(g, None, None, None, m, g.num_nodes, seed=_seed64(seed))
