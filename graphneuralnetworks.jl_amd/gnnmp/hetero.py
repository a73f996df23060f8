"""Heterogeneous graphs: GNNHeteroGraph, the multi-relation aggregation and HeteroGraphConv.

Mirror of the reference (same names, argument meaning and error behaviour):
  GNNHeteroGraph, num_node_types, num_edge_types, edge_type_subgraph     GNNGraphs/src/gnnheterograph/gnnheterograph.jl:103-287
  edge_index(g, et), get_edge_weight(g, et), degree(g, et; dir)          GNNGraphs/src/gnnheterograph/query.jl:9-68
  check_num_nodes / check_num_edges on a heterograph                     GNNGraphs/src/gnnheterograph/utils.jl:1-18
  rand_heterograph, rand_bipartite_heterograph                           GNNGraphs/src/gnnheterograph/generate.jl:42-123
  HeteroGraphConv                                                        GraphNeuralNetworks/src/layers/heteroconv.jl:40-86

A relation (src_t, rel, dst_t) is a bipartite COO edge index with its own cached Plan (n_src = num_nodes[src_t], n_dst =
num_nodes[dst_t]).  What a destination type receives over all of its relations is ONE gnnmp_hetero_propagate_f32 launch for all
destination types (csrc/hetero.hip): the per-relation aggregates are never written.  The composition — propagate per relation, then the
same kernel over identity relations as the combiner — runs instead when a plan has split rows, when the call exceeds the kernel's
relation cap, or when knob 22 (KNOB_HETERO) is negative: the A/B baseline.  Forward only.  GATConv / GATv2Conv members of a
HeteroGraphConv take the attention counterpart of that launch, gnnmp_hetero_attn_f32 (gnnmp/hetero_attn.py, csrc/hetero_attn.hip).

Out of scope: `batch` of heterographs, add_self_loops / add_edges on them, sparse-matrix heterographs.
"""
from __future__ import annotations

import torch

from . import _lib as L
from .graph import Plan, _as_f32, _as_index
from .layers import GraphConv, SAGEConv, dense
from .msgpass import _flat, _fused, aggr_code

_COMBINE = {"+": L.SUM, "max": L.MAX, "min": L.MIN}


def _is_etype(k):
    return isinstance(k, tuple) and len(k) == 3


class GNNHeteroGraph:
    """GNNHeteroGraph(Dict((src_t, rel, dst_t) => (s, t[, w])); num_nodes) — COO storage per relation.

    data       : {(src_t, rel, dst_t): (s, t) | (s, t, w)} (or an iterable of such pairs); indices as GNNGraph holds them
    num_nodes  : {node_t: n}; the default per type is the maximum index seen on that type's side of its relations
    Members: graph, num_nodes, num_edges (dicts), ntypes, etypes (lists, first-appearance order), ndata / edata (dicts, optional).
    """

    is_hetero = True

    def __init__(self, data, num_nodes=None, ndata=None, edata=None, index_base=1, idx_dtype=None, device=None):
        L.require_gpu()
        items = list(data.items()) if isinstance(data, dict) else list(data)
        if not all(_is_etype(k) for k, _ in items):
            raise ValueError("Keys of data must be tuples of the form `(source_type, edge_type, target_type)`")
        self.index_base = int(index_base)
        assert self.index_base in (0, 1)
        dev = None if device is None else torch.device(device)
        self.graph, seen = {}, {}
        for et, v in items:
            assert isinstance(v, (tuple, list)) and len(v) in (2, 3), "a relation is (s, t) or (s, t, w)"
            if dev is None:
                dev = v[0].device if isinstance(v[0], torch.Tensor) and v[0].is_cuda else torch.device("cuda", torch.cuda.current_device())
            s, t = _as_index(v[0], dev), _as_index(v[1], dev)
            if idx_dtype is not None:
                s, t = s.to(idx_dtype), t.to(idx_dtype)
            elif s.dtype != t.dtype:
                t = t.to(s.dtype)
            assert s.dim() == 1 and t.dim() == 1 and s.numel() == t.numel(), "length(s) == length(t)"
            w = _as_f32(v[2], dev) if len(v) == 3 else None
            assert w is None or w.numel() == s.numel(), "length(val) == length(s)"
            self.graph[et] = (s, t, w)
            if s.numel():
                lo = min(int(s.min()), int(t.min()))
                assert lo >= self.index_base, f"relation {et}: index {lo} below the index base {self.index_base}"
                for nt, hi in ((et[0], int(s.max())), (et[2], int(t.max()))):
                    seen[nt] = max(seen.get(nt, 0), hi + 1 - self.index_base)
        self.device = dev if dev is not None else torch.device("cuda", torch.cuda.current_device())
        self.etypes = [et for et, _ in items]
        self.ntypes = []
        for et in self.etypes:
            for nt in (et[0], et[2]):
                if nt not in self.ntypes:
                    self.ntypes.append(nt)
        self.num_nodes = {nt: int((num_nodes or {}).get(nt, seen.get(nt, 0))) for nt in self.ntypes}
        for nt in self.ntypes:      # the index range, asserted at construction (GNNGraphs/src/convert.jl:47-54)
            assert seen.get(nt, 0) <= self.num_nodes[nt], \
                f"node type {nt!r}: index {seen[nt] - 1 + self.index_base} is outside {self.index_base}..{self.num_nodes[nt] - 1 + self.index_base}"
        self.num_edges = {et: int(self.graph[et][0].numel()) for et in self.etypes}
        self.num_graphs = 1
        self.ndata, self.edata = dict(ndata or {}), dict(edata or {})
        for nt, v in self.ndata.items():
            assert v.shape[0] == self.num_nodes[nt]
        for et, v in self.edata.items():
            assert v.shape[0] == self.num_edges[et]
        self._plans = {}      # (et, transposed) -> Plan; shared with every edge_type_subgraph

    # -- queries ------------------------------------------------------------------------------------------------------------------
    @property
    def num_node_types(self):
        return len(self.ntypes)

    @property
    def num_edge_types(self):
        return len(self.etypes)

    def _only(self):
        if len(self.etypes) != 1:
            raise ValueError(f"the graph has {len(self.etypes)} edge types: name one")      # `only` (query.jl:10)
        return self.etypes[0]

    def edge_index(self, et=None):
        return self.graph[self._only() if et is None else et][:2]

    def get_edge_weight(self, et=None):
        return self.graph[self._only() if et is None else et][2]

    def __getitem__(self, key):
        """g[node_t] / g[edge_t]: the features stored for that type (gnnheterograph.jl:289-290)"""
        return self.edata[key] if _is_etype(key) else self.ndata[key]

    @property
    def idx_bytes(self):
        s = next(iter(self.graph.values()))[0]
        return 8 if s.dtype == torch.int64 else 4

    # -- plans (lazy, cached; the index range was asserted at construction) ------------------------------------------------------
    def plan(self, et=None, transposed=False) -> Plan:
        et = self._only() if et is None else et
        p = self._plans.get((et, bool(transposed)))
        if p is None:
            s, t, _ = self.graph[et]
            ns, nd = self.num_nodes[et[0]], self.num_nodes[et[2]]
            p = Plan(t, s, nd, ns, self.index_base, False) if transposed else Plan(s, t, ns, nd, self.index_base, False)
            self._plans[(et, bool(transposed))] = p
        return p

    def plan_transposed(self, et=None) -> Plan:
        return self.plan(et, transposed=True)

    def degree(self, et, T=None, dir="out"):
        """degree(g, edge_type; dir = :out) — query.jl:57-68: out-degrees over num_nodes[src_t], in-degrees over num_nodes[dst_t]"""
        assert dir in ("in", "out")
        plan = self.plan(et, transposed=(dir == "out"))
        deg = torch.empty(plan.n_dst, dtype=torch.float32, device=self.device)
        L.check(L.load().gnnmp_degree_f32(plan.handle, None, L.ptr(deg), L.stream_ptr()))
        T = self.graph[et][0].dtype if T is None else T
        return deg if T == torch.float32 else deg.to(T)

    # -- GNNGraphs/src/gnnheterograph/utils.jl:1-18 ------------------------------------------------------------------------------
    def _check_num_nodes(self, x):
        if x is None:
            return True
        if isinstance(x, dict):
            for nt, v in x.items():
                assert v is None or nt not in self.num_nodes or v.shape[0] == self.num_nodes[nt], \
                    f"Got {v.shape[0]} as last dimension size instead of num_nodes[{nt!r}]={self.num_nodes[nt]}"
            return True
        assert isinstance(x, (tuple, list)) and len(x) == 2, "a heterograph checks a (x_src, x_dst) tuple or a dict by node type"
        src_t, _, dst_t = self._only()
        for v, nt in zip(x, (src_t, dst_t)):
            if isinstance(v, torch.Tensor):
                assert v.shape[0] == self.num_nodes[nt], \
                    f"Got {v.shape[0]} as last dimension size instead of num_nodes[{nt!r}]={self.num_nodes[nt]}"
        return True

    def _check_num_edges(self, e):
        if e is None:
            return True
        if isinstance(e, dict):
            for et, v in e.items():
                assert v is None or v.shape[0] == self.num_edges_of(et), \
                    f"Got {v.shape[0]} as last dimension size instead of num_edges={self.num_edges_of(et)}"
            return True
        if isinstance(e, (tuple, list)):
            return all(self._check_num_edges(v) for v in e)
        n = self.num_edges_of(self._only())
        assert e.shape[0] == n, f"Got {e.shape[0]} as last dimension size instead of num_edges={n}"
        return True

    def num_edges_of(self, et):
        return int(self.graph[et][0].numel())

    def __repr__(self):
        return f"GNNHeteroGraph(num_nodes={self.num_nodes}, num_edges={ {et: self.num_edges_of(et) for et in self.etypes} })"


class HeteroRelation(GNNHeteroGraph):
    """A heterograph of ONE relation — what edge_type_subgraph(g, et) returns and the layers receive.  It answers what the layers and the
    message-passing functions ask of a GNNGraph: plan(), plan_transposed(), s, t, w, num_edges (an integer), index_base, idx_bytes;
    num_nodes stays the dict by node type, and every result has num_nodes[dst_t] rows."""

    def __init__(self, parent, et):
        self.index_base, self.device, self.num_graphs = parent.index_base, parent.device, parent.num_graphs
        self.graph = {et: parent.graph[et]}
        self.etypes = [et]
        self.ntypes = [et[0]] + ([et[2]] if et[2] != et[0] else [])
        self.num_nodes = {nt: parent.num_nodes[nt] for nt in self.ntypes}
        self.ndata = {nt: v for nt, v in parent.ndata.items() if nt in self.ntypes}
        self.edata = {k: v for k, v in parent.edata.items() if k == et}
        self._plans = parent._plans
        self._cache = {}
        self.etype = et
        self.s, self.t, self.w = parent.graph[et]
        self.num_edges = int(self.s.numel())

    def plan(self, add_self_loops=False, transposed=False) -> Plan:
        if _is_etype(add_self_loops):      # plan(et)
            return GNNHeteroGraph.plan(self, add_self_loops, transposed)
        if add_self_loops:
            raise NotImplementedError("add_self_loops on a heterograph relation is out of scope")
        return GNNHeteroGraph.plan(self, self.etype, transposed)

    def plan_transposed(self, add_self_loops=False) -> Plan:
        return self.plan(add_self_loops, transposed=True)


def edge_type_subgraph(g: GNNHeteroGraph, edge_ts):
    """gnnheterograph.jl:250-271.  The subgraph shares g's index arrays and its cached plans."""
    single = _is_etype(edge_ts)
    ets = [edge_ts] if single else list(edge_ts)
    for et in ets:
        assert et in g.etypes, f"Edge type {et} not found in graph"
    if len(ets) == 1:
        return HeteroRelation(g, ets[0])
    sub = object.__new__(GNNHeteroGraph)
    sub.index_base, sub.device, sub.num_graphs = g.index_base, g.device, g.num_graphs
    sub.graph = {et: g.graph[et] for et in ets}
    sub.etypes = ets
    sub.ntypes = []
    for et in ets:
        for nt in (et[0], et[2]):
            if nt not in sub.ntypes:
                sub.ntypes.append(nt)
    sub.num_nodes = {nt: g.num_nodes[nt] for nt in sub.ntypes}
    sub.num_edges = {et: g.num_edges_of(et) for et in ets}
    sub.ndata = {nt: v for nt, v in g.ndata.items() if nt in sub.ntypes}
    sub.edata = {et: v for et, v in g.edata.items() if et in ets}
    sub._plans = g._plans
    return sub


def num_node_types(g):
    return getattr(g, "num_node_types", 1)


def num_edge_types(g):
    return getattr(g, "num_edge_types", 1)


# ---------------------------------------------------------------------------------------------------------
# generators (host side, from a seeded torch CPU generator; no parity with Julia's RNG stream is claimed)
# ---------------------------------------------------------------------------------------------------------
def _rand_edges(gen, n_src, n_dst, m, index_base):
    s = torch.randint(0, max(n_src, 1), (m,), generator=gen, dtype=torch.int64) + index_base
    t = torch.randint(0, max(n_dst, 1), (m,), generator=gen, dtype=torch.int64) + index_base
    return s, t


def rand_heterograph(n, m, bidirected=False, seed=None, **kws):
    """rand_heterograph(n::Dict, m::Dict; bidirected = false) — generate.jl:42-65: m[et] uniform random edges per relation; bidirected:
    the relation (b, r, a) is the reverse of (a, r, b) (the two counts must agree)"""
    gen = torch.Generator(device="cpu")
    gen.manual_seed(0 if seed is None else int(seed))
    base = int(kws.get("index_base", 1))
    graphs = {}
    for et in m:
        if et in graphs:
            continue
        rev = (et[2], et[1], et[0])
        if bidirected and rev != et:
            assert rev in m and m[et] == m[rev], "Number of edges must be the same in reverse edge types for bidirected graphs."
        s, t = _rand_edges(gen, n[et[0]], n[et[2]], int(m[et]), base)
        graphs[et] = (s, t)
        if bidirected and rev != et:
            graphs[rev] = (t.clone(), s.clone())
    return GNNHeteroGraph({et: graphs[et] for et in m}, num_nodes=dict(n), **kws)


def rand_bipartite_heterograph(n, m, bidirected=True, node_t=("A", "B"), edge_t="to", seed=None, **kws):
    """rand_bipartite_heterograph((n1, n2), m | (m1, m2); bidirected = true, node_t = (:A, :B), edge_t = :to) — generate.jl:112-123"""
    n1, n2 = n
    m1, m2 = (m, m) if isinstance(m, int) else m
    if bidirected:
        assert m1 == m2, "bidirected: the two edge counts must agree"
    a, b = node_t
    return rand_heterograph({a: n1, b: n2}, {(a, edge_t, b): m1, (b, edge_t, a): m2}, bidirected=bidirected, seed=seed, **kws)


# ---------------------------------------------------------------------------------------------------------
# the aggregation
# ---------------------------------------------------------------------------------------------------------
def _use_fused_kernel():
    return L.knob(L.KNOB_HETERO) >= 0


def _hetero_call(records, D):
    """ONE gnnmp_hetero_propagate_f32 call.  records: [(out, n_dst, combine code, [(Plan | None, x, w | None, aggr code)])]"""
    dsts = (L.HeteroDst * len(records))()
    keep = []
    for d, (out, n_dst, combine, rels) in zip(dsts, records):
        tab = (L.HeteroRel * len(rels))()
        for r, (plan, x, w, aggr) in zip(tab, rels):
            r.plan = None if plan is None else plan.handle
            r.x, r.w, r.aggr = x.data_ptr() or None, None if w is None else w.data_ptr(), aggr
        keep.append(tab)
        d.out, d.n_dst, d.combine, d.n_rel, d.rels = out.data_ptr() or None, n_dst, combine, len(rels), tab
    L.check(L.load().gnnmp_hetero_propagate_f32(dsts, len(records), D, L.stream_ptr()))


def _combine(groups, combine, D):
    """{dst_t: [tensor [n_dst, D], ...]} -> {dst_t: foldl(combine, tensors)} by the kernel's identity relations: one call for as many
    destination types as fit the relation cap; a type with more terms than the cap folds in several calls, its running value first"""
    out, pending, used = {}, [], 0

    def flush():
        nonlocal pending, used
        if pending:
            _hetero_call(pending, D)
        pending, used = [], 0

    for dst_t, terms in groups.items():
        terms = list(terms)
        while len(terms) > 1:
            room = L.HETERO_MAX_REL - used
            if room < 2:
                flush()
                continue
            take, terms = terms[:room], terms[room:]
            y = torch.empty_like(take[0])
            pending.append((y, y.shape[0], combine, [(None, t, None, L.SUM) for t in take]))
            used += len(take)
            if terms:                      # more to fold: the running value leads the next call
                flush()
            terms = [y] + terms
        out[dst_t] = terms[0]
    flush()
    return out


def _dst_groups(etypes):
    groups = {}
    for et in etypes:
        groups.setdefault(et[2], []).append(et)
    return groups


def hetero_propagate(g: GNNHeteroGraph, x, aggr="+", combine="+", edge_weight=None, root=None):
    """For every destination type: foldl(combine, [root[dst_t],] m_1, ..., m_R) with m_r = propagate(copy_xj | w_mul_xj, g_r, aggr_r; xj =
    x[src_t]) over the relations that arrive at it, in g.etypes order.  x: {node_t: [n, D]}; aggr: a string, or {edge_t: string};
    combine: "+", "max" or "min"; edge_weight: {edge_t: [E]} (those relations use w_mul_xj), True (the graph's own weights where it has
    them) or None; root: {dst_t: [n_dst, D]} entering the fold first.  Returns {dst_t: [n_dst, D]}."""
    if combine not in _COMBINE:
        raise ValueError(f"combine must be '+', 'max' or 'min' (got {combine!r})")
    g._check_num_nodes(x)
    ccode = _COMBINE[combine]
    recs, D = {}, None      # {dst_t: [(edge_t | None, Plan | None, x, w, aggr code)]}
    for dst_t, ets in _dst_groups(g.etypes).items():
        rels = []
        if root is not None and root.get(dst_t) is not None:
            r = _flat(root[dst_t])
            assert r.shape[0] == g.num_nodes[dst_t]
            rels.append((None, None, r, None, L.SUM))
        for et in ets:
            w = g.graph[et][2] if edge_weight is True else (edge_weight or {}).get(et)
            if w is not None:
                w = _as_f32(w, g.device)
                assert w.numel() == g.num_edges_of(et), f"Got {w.numel()} edge weights instead of num_edges={g.num_edges_of(et)}"
            rels.append((et, g.plan(et), _flat(x[et[0]]), w, aggr_code(aggr[et] if isinstance(aggr, dict) else aggr)))
        recs[dst_t] = rels
        for rel in rels:
            D = rel[2].shape[1] if D is None else D
            assert rel[2].shape[1] == D, "every relation of a call aggregates rows of one width"
    if not recs:
        return {}
    n_records = sum(len(r) for r in recs.values())
    split = any(rel[1] is not None and rel[1].n_long > 0 for r in recs.values() for rel in r)
    if _use_fused_kernel() and not split and n_records <= L.HETERO_MAX_REL:
        out = {t: torch.empty((g.num_nodes[t], D), dtype=torch.float32, device=g.device) for t in recs}
        _hetero_call([(out[t], g.num_nodes[t], ccode, [rel[1:] for rel in recs[t]]) for t in recs], D)
        return out
    # the composition: propagate per relation (split rows take the chunked row kernel), then the identity-relation combiner
    terms = {}
    for dst_t, rels in recs.items():
        terms[dst_t] = [xs if et is None else _fused(edge_type_subgraph(g, et), L.COPY_XJ if w is None else L.W_MUL_XJ, _AGGR_NAME[code], xs, w)
                        for et, _, xs, w, code in rels]
    return _combine(terms, ccode, D)


_AGGR_NAME = {L.SUM: "+", L.MEAN: "mean", L.MAX: "max", L.MIN: "min"}


# ---------------------------------------------------------------------------------------------------------
# HeteroGraphConv
# ---------------------------------------------------------------------------------------------------------
# layers whose functional body takes (x_src, x_dst) through expand_srcdst: they run on a bipartite relation as they are
_BIPARTITE_LAYERS = (GraphConv, SAGEConv)


def _add(a, b):
    out = torch.empty_like(a)
    L.check(L.load().gnnmp_add_f32(L.ptr(a), L.ptr(b), L.ptr(out), a.numel(), L.stream_ptr()))
    return out


def _split_weights(l, Din):
    """(W_root, W_agg) of a GraphConv / SAGEConv"""
    if isinstance(l, GraphConv):
        return l.weight1, l.weight2
    return l.weight[:, :Din], l.weight[:, Din:]


class HeteroGraphConv:
    """HeteroGraphConv(itr; aggr = +) — heteroconv.jl:40-55.  itr: {edge_t: layer} or an iterable of (edge_t, layer) pairs; aggr: "+",
    "max" or "min" (the fold over the outputs that arrive at one destination type).  layer(g, x) with x a dict by node type returns a
    dict keyed by the destination types, in first-appearance order."""

    def __init__(self, itr, aggr="+"):
        pairs = list(itr.items()) if isinstance(itr, dict) else list(itr)
        if aggr not in _COMBINE:
            raise ValueError(f"HeteroGraphConv: aggr must be '+', 'max' or 'min' (got {aggr!r})")
        self.etypes = [et for et, _ in pairs]
        self.layers = [l for _, l in pairs]
        self.aggr = aggr

    def _fusable(self, members, x):
        """the transform-first path for one destination type: every incoming layer is a GraphConv / SAGEConv without activation that
        aggregates with + or mean, Dout <= Din (gcn_conv's W-first rule, GNNlib/src/layers/conv.jl:36-40), and the fold is +"""
        if self.aggr != "+" or not _use_fused_kernel():
            return False
        for et, l in members:
            if not isinstance(l, _BIPARTITE_LAYERS) or l.sigma is not None or l.aggr not in ("+", "sum", "mean"):
                return False
            Din = x[et[0]].shape[1]
            if _split_weights(l, Din)[0].shape[0] > Din or x[et[2]].shape[1] != Din:
                return False
        return True

    def __call__(self, g: GNNHeteroGraph, x):
        g._check_num_nodes(x)
        by_dst = {}
        for et, l in zip(self.etypes, self.layers):
            by_dst.setdefault(et[2], []).append((et, l))
        from .hetero_attn import Projections, fused_records, hetero_attn_batches
        fused, outs, attn = {}, {}, {}
        proj = Projections(x)      # a projection several relations share (same layer object, same node type) is computed once
        for dst_t, members in by_dst.items():
            plans = [g.plan(et) for et, _ in members]
            recs = fused_records(members, plans, proj)
            if recs is not None:      # attention members: ONE gnnmp_hetero_attn_f32 launch per (heads, out), below
                attn.setdefault(recs[0], []).append((dst_t, recs[1]))
            elif self._fusable(members, x) and all(p.n_long == 0 for p in plans) and len(members) + 1 <= L.HETERO_MAX_REL:
                # by linearity: Σ_r (W_root_r x_dst + W_agg_r A_r x_src_r + b_r) = (Σ W_root_r) x_dst + Σ b_r + Σ_r A_r (W_agg_r x_src_r)
                W_root = bias = None
                rels = []
                for (et, l), p in zip(members, plans):
                    xs = _flat(x[et[0]])
                    wr, wa = _split_weights(l, xs.shape[1])
                    wr = wr.contiguous()
                    W_root = wr if W_root is None else _add(W_root, wr)
                    if l.bias is not None:
                        bias = l.bias if bias is None else _add(bias, l.bias)
                    rels.append((p, dense(xs, wa), None, aggr_code(l.aggr)))
                rootv = dense(_flat(x[dst_t]), W_root, bias)
                fused[dst_t] = [(None, rootv, None, L.SUM)] + rels
            else:
                outs[dst_t] = [self._forward(l, g, et, x) for et, l in members]
        result = {}
        for (H, C), group in attn.items():
            recs = []
            for dst_t, rels in group:
                result[dst_t] = torch.empty((g.num_nodes[dst_t], H * C), dtype=torch.float32, device=g.device)
                recs.append((result[dst_t], g.num_nodes[dst_t], _COMBINE[self.aggr], rels))
            hetero_attn_batches(recs, H, C)
        if fused:      # ONE launch for the fused destination types (one per output width, as far as the relation cap allows)
            recs = []
            for dst_t, rels in fused.items():
                result[dst_t] = torch.empty_like(rels[0][1])
                recs.append((result[dst_t], result[dst_t].shape[0], L.SUM, rels))
            for D in sorted({r[0].shape[1] for r in recs}):
                batch, used = [], 0
                for r in (r for r in recs if r[0].shape[1] == D):
                    if used + len(r[3]) > L.HETERO_MAX_REL:
                        _hetero_call(batch, D)
                        batch, used = [], 0
                    batch.append(r)
                    used += len(r[3])
                _hetero_call(batch, D)
        for D in sorted({ys[0].shape[1] for ys in outs.values()}):
            result.update(_combine({t: ys for t, ys in outs.items() if ys[0].shape[1] == D}, _COMBINE[self.aggr], D))
        return {dst_t: result[dst_t] for dst_t in by_dst}

    @staticmethod
    def _forward(l, g, et, x):
        from .hetero_attn import is_attention_layer
        if not isinstance(l, _BIPARTITE_LAYERS) and not is_attention_layer(l):
            raise NotImplementedError(f"HeteroGraphConv: {type(l).__name__} does not take a (x_src, x_dst) pair on a bipartite relation "
                                      "(supported: GraphConv, SAGEConv, GATConv, GATv2Conv)")
        return l(edge_type_subgraph(g, et), (x[et[0]], x[et[2]]))
