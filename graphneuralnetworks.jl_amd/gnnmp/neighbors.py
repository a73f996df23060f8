"""Graph constructors from point clouds: knn_graph and radius_graph (GNNGraphs/src/generate.jl:112-145, 196-222).

The reference searches NearestNeighbors.jl trees on the CPU; here the search is an exact brute-force kernel (csrc/neighbors.hip,
include/gnnmp.h states the semantics: fp32 fma chain, ties to the lower index, `self_loops=False` excludes a node by index, the
candidates of a node are the nodes of its graph on the raw coordinates).  torch allocates; the indices are libgnnmp's.

The edges come out destination-sorted (edge i k + r joins centre i and its r-th neighbour), so the two entry points write the
graph's PLAN themselves — no sort, no gnnmp_plan_create on first use — and (s, t) are read off it by gnnmp_plan_edge_index in the
index width and base asked for.  The calls synchronise the stream, as every plan build does.  dir="in": that plan is the graph's;
dir="out": it is the plan of the reversed edges (plan_transposed), and the graph's own plan is built on first use as usual.
"""
from __future__ import annotations

import ctypes
import math

import torch

from . import _lib as L
from .graph import GNNGraph, Plan, _as_f32, _as_index

MAX_K = 1024


def _prepare(points, graph_indicator, dir, index_base, idx_dtype):
    L.require_gpu()
    assert dir in ("in", "out"), "dir must be :in or :out"            # GNNGraph(adj_list; dir), convert.jl:97
    assert index_base in (0, 1)
    assert idx_dtype in (torch.int64, torch.int32)
    device = points.device if isinstance(points, torch.Tensor) and points.is_cuda else torch.device("cuda", torch.cuda.current_device())
    x = _as_f32(points, device)
    assert x.dim() == 2, "points is a (num_nodes, num_features) matrix"
    n = int(x.shape[0])
    gi, G = None, 1
    if graph_indicator is not None:
        gi = graph_indicator if isinstance(graph_indicator, torch.Tensor) else torch.as_tensor(graph_indicator)
        assert not gi.dtype.is_floating_point and gi.dtype != torch.bool, "graph_indicator isa AbstractVector{<:Integer}"
        gi = _as_index(gi, device)
        assert gi.dim() == 1 and gi.numel() == n, "length(graph_indicator) == n"
        G = (int(gi.max()) + 1 - index_base) if n > 0 else 1          # num_graphs = maximum(graph_indicator), gnngraph.jl:138
        assert n == 0 or (int(gi.min()) >= index_base), "graph_indicator below the index base"
    return x, n, gi, G, device


def _status(rc):
    if rc == L.EBOUNDS:                                               # the reference's @assert (generate.jl:123)
        raise AssertionError(L.load().gnnmp_last_error().decode())
    if rc == L.EINVAL:
        raise ValueError(L.load().gnnmp_last_error().decode())
    L.check(rc)


def _own_plan(handle, device) -> Plan:
    """a Plan object around a handle the library made for the caller (destroyed with the object, like Plan.from_csc's)"""
    p = object.__new__(Plan)
    p._lib = L.load()
    p._h = handle
    info = (ctypes.c_int64 * 8)()
    L.check(p._lib.gnnmp_plan_info(p._h, info))
    p.n_src, p.n_dst, p.n_edges, p.n_total = info[0], info[1], info[2], info[3]
    p.max_degree, p.n_long, p.bytes, p.long_thresh = info[4], info[5], info[6], info[7]
    p.device = device
    return p


def _graph(handle, n, gi, G, dir, index_base, idx_dtype, device, kws):
    plan = _own_plan(handle, device)
    nb, centre = plan.edge_index(idx_dtype, index_base)              # adjacency list -> COO (convert.jl:97-117)
    s, t = (nb, centre) if dir == "in" else (centre, nb)
    g = GNNGraph(s, t, num_nodes=n, graph_indicator=gi, num_graphs=G, index_base=index_base, device=device, _validated=True, **kws)
    g._plans[False if dir == "in" else ("T", False)] = plan
    return g


def _indicator_args(gi, index_base, G):
    return L.ptr(gi), (0 if gi is None else gi.element_size()), index_base, G


def knn_graph(points, k, graph_indicator=None, self_loops=False, dir="in", index_base=1, idx_dtype=torch.int64, **kws) -> GNNGraph:
    """knn_graph(points, k; graph_indicator = nothing, self_loops = false, dir = :in, kws...) — generate.jl:112-145: every node is
    linked to its k nearest points (of its own graph when graph_indicator is given: a batch, num_graphs = max(graph_indicator)).
    points: (num_nodes, num_features) float32.  Edge i k + r joins node i and its r-th nearest neighbour (ties: lower index);
    dir="in": neighbour -> node.  A graph with fewer than k (k + 1 without self loops) nodes: AssertionError.  kws go to GNNGraph."""
    k = int(k)
    if k < 1 or k > MAX_K:
        raise ValueError(f"knn_graph: k = {k} outside 1..{MAX_K}")
    x, n, gi, G, device = _prepare(points, graph_indicator, dir, index_base, idx_dtype)
    if x.shape[1] < 1:
        raise ValueError("knn_graph: points have no features")
    h = ctypes.c_void_p()
    _status(L.load().gnnmp_knn_graph_f32(ctypes.byref(h), L.ptr(x), n, x.shape[1], k, *_indicator_args(gi, index_base, G),
                                         int(bool(self_loops)), L.stream_ptr()))
    return _graph(h, n, gi, G, dir, index_base, idx_dtype, device, kws)


def radius_graph(points, r, graph_indicator=None, self_loops=False, dir="in", index_base=1, idx_dtype=torch.int64, **kws) -> GNNGraph:
    """radius_graph(points, r; graph_indicator = nothing, self_loops = false, dir = :in, kws...) — generate.jl:196-222: every node is
    linked to the points (of its own graph) within distance r: d2 <= r^2 in float32.  Nodes ascend, the neighbours of a node ascend."""
    r = float(r)
    if not r >= 0.0 or math.isnan(r):
        raise ValueError(f"radius_graph: r = {r} (negative or NaN)")
    x, n, gi, G, device = _prepare(points, graph_indicator, dir, index_base, idx_dtype)
    if x.shape[1] < 1:
        raise ValueError("radius_graph: points have no features")
    h = ctypes.c_void_p()
    _status(L.load().gnnmp_radius_graph_f32(ctypes.byref(h), L.ptr(x), n, x.shape[1], ctypes.c_float(r),
                                            *_indicator_args(gi, index_base, G), int(bool(self_loops)), L.stream_ptr()))
    return _graph(h, n, gi, G, dir, index_base, idx_dtype, device, kws)
