"""Adjoints of the heterograph aggregation and of HeteroGraphConv (gnnmp/hetero.py), on the HIP kernels.

The backward of a heterogeneous layer has the forward's shape, mirrored: what a SOURCE type receives is a sum over all relations that
leave it.  That sum is ONE gnnmp_hetero_propagate_grad_f32 launch for all source types (csrc/hetero_backward.hip): a lane group owns a
source row, walks it in every outgoing relation's transposed plan and stores Δx once.  Per relation the walk is
  + / mean (copy_xj | w_mul_xj)   Σ w_k * (Δ[t_k] * 1/count[t_k])            — NNlib: ∇scatter(+ | mean) = gather (./ count), ∇gather = scatter(+)
  max / min (copy_xj)             Σ (x[j] == y[t_k]) ? Δ[t_k] : 0            — NNlib: ∇scatter(max | min), every tie receives Δ
and a term that is no walk (a layer's root term) enters as an identity relation.  The fold over the relations of one destination type,
foldl(max | min, terms), is pulled back by the same export's masked-identity mode: Δterm = (term .== out) .* Δout (every tying term
receives Δ: this project's rule, see include/gnnmp.h).  Δw of a weighted relation is the existing edge-wise dot product
(gnnmp_edge_dot_plan_f32 / gnnmp_edge_dot_f32).

The composition — per relation gnnmp_propagate_f32 on the transposed plan or gnnmp_propagate_maxmin_grad_f32, summed by the forward
kernel's identity relations — runs instead when a transposed plan has split rows, when a call exceeds the kernel's relation cap, or
when knob 22 (KNOB_HETERO) is negative: the A/B baseline.

  hetero_propagate_grad(g, dy, ...)     {node_t: Δx} of hetero_propagate(..., combine = "+")
  hetero_propagate_ad(g, x, ...)        differentiable hetero_propagate: gradients to x, root and the edge weights
  hetero_conv_ad(layer, g, x)           differentiable HeteroGraphConv of GraphConv / SAGEConv members, σ in identity, relu — or of GATConv /
                                        GATv2Conv members (gnnmp/hetero_attn.py)

Out of scope: Float64, `batch` of heterographs, a fused ΔW.
"""
from __future__ import annotations

import torch

from . import _lib as L
from .backward import _act_code, act_grad, dense_grad_w, dense_grad_x, propagate_grad_w
from .graph import _as_f32
from .hetero import (_AGGR_NAME, _BIPARTITE_LAYERS, _COMBINE, GNNHeteroGraph, _combine, _dst_groups, _hetero_call, _split_weights,
                     _use_fused_kernel, edge_type_subgraph)
from .layers import dense
from .msgpass import _flat, _fused, aggr_code


def _grad_call(records, D):
    """ONE gnnmp_hetero_propagate_grad_f32 call.  records: [(dx, x | None, n_src, [(Plan (transposed) | None, dy, w, sd, y, out)])]"""
    srcs = (L.HeteroSrc * len(records))()
    keep = []
    p = lambda t: None if t is None else (t.data_ptr() or None)      # noqa: E731
    for s, (dx, x, n_src, rels) in zip(srcs, records):
        tab = (L.HeteroRelGrad * len(rels))()
        for r, (plan_t, dy, w, sd, y, out) in zip(tab, rels):
            r.plan_t = None if plan_t is None else plan_t.handle
            r.dy, r.w, r.sd, r.y, r.out = p(dy), p(w), p(sd), p(y), p(out)
        keep.append(tab)
        s.dx, s.x, s.n_src, s.n_rel, s.rels = p(dx), p(x), n_src, len(rels), tab
    L.check(L.load().gnnmp_hetero_propagate_grad_f32(srcs, len(records), D, L.stream_ptr()))


def _inv_count(g: GNNHeteroGraph, et):
    """1 / max(in-degree, 1) of relation et's destinations: the factor of ∇scatter(mean); a constant of the graph, cached on it"""
    cache = g.__dict__.setdefault("_inv_count", {})
    inv = cache.get(et)
    if inv is None:
        cnt = torch.empty(g.num_nodes[et[2]], dtype=torch.float32, device=g.device)
        L.check(L.load().gnnmp_degree_f32(g.plan(et).handle, None, L.ptr(cnt), L.stream_ptr()))
        inv = cache[et] = torch.reciprocal(torch.clamp(cnt, min=1.0))
    return inv


def _scale_rows(v, m):
    """out[i][:] = v[i] * m[i][:]"""
    out = torch.empty_like(m)
    L.check(L.load().gnnmp_mul_rows_f32(L.ptr(v), 1, L.ptr(m), L.ptr(out), m.shape[0], m.shape[1], L.stream_ptr()))
    return out


def _edge_weight(g, et, edge_weight):
    w = g.graph[et][2] if edge_weight is True else (edge_weight or {}).get(et)
    if w is not None:
        w = _as_f32(w, g.device)
        assert w.numel() == g.num_edges_of(et), f"Got {w.numel()} edge weights instead of num_edges={g.num_edges_of(et)}"
    return w


def _src_grad(g: GNNHeteroGraph, per_src, x, D):
    """{src_t: Σ terms} — terms in order, each ("id", None, dy, None, None, None) | ("lin", edge_t, dy, w | None, sd | None, None) |
    ("win", edge_t, dy, None, None, y).  One launch for all source types, or the composition (module docstring)."""
    plans = {t[1]: g.plan(t[1], transposed=True) for terms in per_src.values() for t in terms if t[0] != "id"}
    n_records = sum(len(terms) for terms in per_src.values())
    split = any(p.n_long > 0 for p in plans.values())
    f32 = dict(dtype=torch.float32, device=g.device)
    if _use_fused_kernel() and not split and n_records <= L.HETERO_MAX_REL:
        out = {s: torch.empty((g.num_nodes[s], D), **f32) for s in per_src}
        recs = []
        for s, terms in per_src.items():
            xs = _flat(x[s]) if any(t[0] == "win" for t in terms) else None
            recs.append((out[s], xs, g.num_nodes[s], [(plans.get(et), dy, w, sd, y, None) for _, et, dy, w, sd, y in terms]))
        _grad_call(recs, D)
        return out
    lib = L.load()
    mats = {}
    for s, terms in per_src.items():
        mats[s] = []
        for kind, et, dy, w, sd, y in terms:
            if kind == "id":
                mats[s].append(dy)
                continue
            dx = torch.empty((g.num_nodes[s], D), **f32)
            if kind == "win":
                L.check(lib.gnnmp_propagate_maxmin_grad_f32(plans[et].handle, L.ptr(_flat(x[s])), L.ptr(y), L.ptr(dy), L.ptr(dx), D,
                                                            L.stream_ptr()))
            else:       # the forward kernel on the reversed edges; 1/count rides as the factor of the gathered row (propagate_grad_xj)
                L.check(lib.gnnmp_propagate_f32(plans[et].handle, L.COPY_XJ if w is None else L.W_MUL_XJ, L.SUM, L.ptr(dy), L.ptr(w),
                                                L.ptr(sd), None, L.ptr(dx), D, L.stream_ptr()))
            mats[s].append(dx)
    return _combine(mats, L.SUM, D)


def _fold_grad(groups, D):
    """the pullback of out = foldl(max | min, terms): [(out, Δout, [term, ...])] -> [[Δterm, ...]] by the masked-identity mode, every term
    a record of its own: one launch per HETERO_MAX_REL terms.  A fold of one term hands Δout through."""
    res, pending = [], []
    for out, dout, terms in groups:
        if len(terms) == 1:
            res.append([dout])
            continue
        ds = [torch.empty_like(dout) for _ in terms]
        pending += [(d, None, d.shape[0], [(None, dout, None, None, t, out)]) for d, t in zip(ds, terms)]
        res.append(ds)
    for k in range(0, len(pending), L.HETERO_MAX_REL):
        _grad_call(pending[k:k + L.HETERO_MAX_REL], D)
    return res


def hetero_propagate_grad(g: GNNHeteroGraph, dy, x=None, aggr="+", edge_weight=None, saved=None):
    """Δx of hetero_propagate(g, x, aggr, "+", edge_weight): {node_t: [n, D]} for every node type of g (zeros for a type that is no
    relation's source).  dy: {dst_t: Δ [n_dst, D]}; a max / min relation needs the forward input x: {node_t: [n, D]} and its forward
    aggregate saved: {edge_t: [n_dst, D]}."""
    per_src, D = {}, None
    for et in g.etypes:
        if dy.get(et[2]) is None:
            continue
        d = _flat(dy[et[2]])
        assert d.shape[0] == g.num_nodes[et[2]]
        D = d.shape[1] if D is None else D
        assert d.shape[1] == D, "every relation of a call aggregates rows of one width"
        code = aggr_code(aggr[et] if isinstance(aggr, dict) else aggr)
        w = _edge_weight(g, et, edge_weight)
        if code in (L.MAX, L.MIN):
            if w is not None:
                raise ValueError("the max / min adjoint is implemented for copy_xj (no edge weights)")
            if x is None or saved is None or saved.get(et) is None:
                raise ValueError(f"relation {et}: the max / min adjoint needs the forward input x and the forward aggregate saved[edge_t]")
            term = ("win", et, d, None, None, _flat(saved[et]))
        else:
            term = ("lin", et, d, w, _inv_count(g, et) if code == L.MEAN else None, None)
        per_src.setdefault(et[0], []).append(term)
    if D is None:
        return {}
    out = _src_grad(g, per_src, x, D)
    return {nt: out[nt] if nt in out else torch.zeros((g.num_nodes[nt], D), dtype=torch.float32, device=g.device) for nt in g.ntypes}


# ---------------------------------------------------------------------------------------------------------
# hetero_propagate as an autograd function
# ---------------------------------------------------------------------------------------------------------
class _HeteroPropagateFn(torch.autograd.Function):
    """inputs: x by node type, root by destination type, w by edge type (spec names them); outputs: one tensor per destination type"""

    @staticmethod
    def forward(ctx, g, spec, *tensors):
        x_keys, root_keys, w_keys, aggr, combine = spec
        nx, nr = len(x_keys), len(root_keys)
        x = {k: _flat(t) for k, t in zip(x_keys, tensors[:nx])}
        root = {k: _flat(t) for k, t in zip(root_keys, tensors[nx:nx + nr])}
        ws = {k: t.contiguous() for k, t in zip(w_keys, tensors[nx + nr:])}
        ccode = _COMBINE[combine]
        groups = _dst_groups(g.etypes)
        D = next(iter(x.values())).shape[1]
        n_records = len(g.etypes) + sum(1 for t in groups if t in root)
        lin = [et for et in g.etypes if aggr[et] in (L.SUM, L.MEAN)]
        one_launch = combine == "+" and _use_fused_kernel() and n_records <= L.HETERO_MAX_REL and all(g.plan(et).n_long == 0 for et in lin)
        terms = {}      # {dst_t: [(edge_t | None, materialised term | None)]}: root first, then the relations in g.etypes order
        for dst_t, ets in groups.items():
            ts = [(None, root[dst_t])] if dst_t in root else []
            for et in ets:
                # a max / min relation is always computed by propagate: its aggregate is what the winners mode of the pullback compares
                # against, and it enters the fold as an identity relation
                m = None
                if not one_launch or aggr[et] in (L.MAX, L.MIN):
                    w = ws.get(et)
                    m = _fused(edge_type_subgraph(g, et), L.COPY_XJ if w is None else L.W_MUL_XJ, _AGGR_NAME[aggr[et]], x[et[0]], w)
                ts.append((et, m))
            terms[dst_t] = ts
        if one_launch:
            out = {t: torch.empty((g.num_nodes[t], D), dtype=torch.float32, device=g.device) for t in terms}
            _hetero_call([(out[t], g.num_nodes[t], ccode,
                           [(None, m, None, L.SUM) if m is not None else (g.plan(et), x[et[0]], ws.get(et), aggr[et]) for et, m in ts])
                          for t, ts in terms.items()], D)
        else:
            out = _combine({t: [m for _, m in ts] for t, ts in terms.items()}, ccode, D)
        ctx.g, ctx.spec, ctx.D = g, spec, D
        ctx.layout = {t: [et for et, _ in ts] for t, ts in terms.items()}
        mats = [m for ts in terms.values() for et, m in ts if et is not None and m is not None]
        ctx.has_mat = {et: m is not None for ts in terms.values() for et, m in ts if et is not None}
        ctx.save_for_backward(*x.values(), *root.values(), *ws.values(), *mats, *out.values())
        return tuple(out[t] for t in terms)

    @staticmethod
    def backward(ctx, *douts):
        g, D = ctx.g, ctx.D
        x_keys, root_keys, w_keys, aggr, combine = ctx.spec
        nx, nr, nw = len(x_keys), len(root_keys), len(w_keys)
        saved = ctx.saved_tensors
        x = dict(zip(x_keys, saved[:nx]))
        root = dict(zip(root_keys, saved[nx:nx + nr]))
        ws = dict(zip(w_keys, saved[nx + nr:nx + nr + nw]))
        n_mat = sum(ctx.has_mat.values())
        mats = dict(zip([et for et, has in ctx.has_mat.items() if has], saved[nx + nr + nw:nx + nr + nw + n_mat]))
        outs = dict(zip(ctx.layout, saved[nx + nr + nw + n_mat:]))
        douts = {t: d.contiguous() for t, d in zip(ctx.layout, douts)}
        # Δ per term of every fold
        if combine == "+":
            dterm = {t: [douts[t]] * len(ets) for t, ets in ctx.layout.items()}
        else:
            folds = [(outs[t], douts[t], [root[t] if et is None else mats[et] for et in ets]) for t, ets in ctx.layout.items()]
            dterm = dict(zip(ctx.layout, _fold_grad(folds, D)))
        droot, dw, per_src = {}, {}, {}
        for t, ets in ctx.layout.items():
            for et, d in zip(ets, dterm[t]):
                if et is None:
                    droot[t] = d
                    continue
                code, w = aggr[et], ws.get(et)
                if code in (L.MAX, L.MIN):
                    term = ("win", et, d, None, None, mats[et])
                else:
                    inv = _inv_count(g, et) if code == L.MEAN else None
                    term = ("lin", et, d, w, inv, None)
                    if w is not None:      # Δw[k] = Δ[t_k] · x[s_k]; for mean Δ is pre-scaled by 1 / count, as _PropagateFn does
                        dw[et] = propagate_grad_w(edge_type_subgraph(g, et), d if inv is None else _scale_rows(inv, d), x[et[0]])
                per_src.setdefault(et[0], []).append(term)
        # (edge types in g.etypes order per source type: the table order of the sum)
        per_src = {s: sorted(ts, key=lambda t: g.etypes.index(t[1])) for s, ts in per_src.items()}
        dx = _src_grad(g, per_src, x, D) if any(ctx.needs_input_grad[2:2 + nx]) else {}
        gx = [dx[k].view(saved[i].shape) if k in dx else torch.zeros_like(saved[i]) for i, k in enumerate(x_keys)]
        return (None, None, *gx, *[droot[k] for k in root_keys], *[dw[k] for k in w_keys])


def hetero_propagate_ad(g: GNNHeteroGraph, x, aggr="+", combine="+", edge_weight=None, root=None):
    """differentiable hetero_propagate (same arguments, same result): gradients to every x[node_t], every root[dst_t] and every
    edge-weight vector — forward and backward both on the HIP kernels"""
    if combine not in _COMBINE:
        raise ValueError(f"combine must be '+', 'max' or 'min' (got {combine!r})")
    codes = {et: aggr_code(aggr[et] if isinstance(aggr, dict) else aggr) for et in g.etypes}
    ws = {et: w for et in g.etypes if (w := _edge_weight(g, et, edge_weight)) is not None}
    for et in ws:
        if codes[et] in (L.MAX, L.MIN):
            raise ValueError(f"relation {et}: the max / min adjoint is implemented for copy_xj (no edge weights)")
    g._check_num_nodes(x)
    groups = _dst_groups(g.etypes)
    rows = lambda v: v if v.dim() == 2 else v.reshape(v.shape[0], -1)      # noqa: E731
    x = {k: rows(v) for k, v in x.items() if k in g.num_nodes}
    root = {k: rows(v) for k, v in (root or {}).items() if v is not None and k in groups}
    if not groups:
        return {}
    D = {v.shape[1] for v in list(x.values()) + list(root.values())}
    assert len(D) == 1, "every relation of a call aggregates rows of one width"
    for k, v in root.items():
        assert v.shape[0] == g.num_nodes[k]
    spec = (tuple(x), tuple(root), tuple(ws), codes, combine)
    out = _HeteroPropagateFn.apply(g, spec, *x.values(), *root.values(), *ws.values())
    return dict(zip(groups, out))


# ---------------------------------------------------------------------------------------------------------
# HeteroGraphConv as an autograd function
# ---------------------------------------------------------------------------------------------------------
class _HeteroConvFn(torch.autograd.Function):
    """y_d = foldl(aggr, [σ_r.(W_root_r x_d + W_agg_r m_r + b_r) for r into d]), m_r = propagate(copy_xj, g_r, aggr_r; xj = x_src).
    inputs: x by node type, then (W_root, W_agg, b) per member; outputs: one tensor per destination type"""

    @staticmethod
    def forward(ctx, g, spec, *tensors):
        x_keys, members, combine = spec          # members: [(edge_t, σ, aggr name)]
        nx = len(x_keys)
        x = {k: _flat(t) for k, t in zip(x_keys, tensors[:nx])}
        params = tensors[nx:]
        ms, ys, by_dst = [], [], {}
        for k, (et, sigma, aggr) in enumerate(members):
            wr, wa, b = params[3 * k:3 * k + 3]
            m = _fused(edge_type_subgraph(g, et), L.COPY_XJ, aggr, x[et[0]], None)      # saved: the ΔW_agg operand (and max / min's y)
            ms.append(m)
            ys.append(dense(x[et[2]], wr, b, sigma, x2=m, W2=wa))
            by_dst.setdefault(et[2], []).append(k)
        out = {}
        for D in sorted({ys[ks[0]].shape[1] for ks in by_dst.values()}):
            out.update(_combine({t: [ys[k] for k in ks] for t, ks in by_dst.items() if ys[ks[0]].shape[1] == D}, _COMBINE[combine], D))
        ctx.g, ctx.spec, ctx.by_dst = g, spec, by_dst
        ctx.save_for_backward(*x.values(), *params, *ms, *ys, *[out[t] for t in by_dst])
        return tuple(out[t] for t in by_dst)      # (a destination type with ONE member: its output is that member's y itself)

    @staticmethod
    def backward(ctx, *douts):
        g, by_dst = ctx.g, ctx.by_dst
        x_keys, members, combine = ctx.spec
        nx, R = len(x_keys), len(members)
        saved = ctx.saved_tensors
        x = dict(zip(x_keys, saved[:nx]))
        params = saved[nx:nx + 3 * R]
        ms, ys = saved[nx + 3 * R:nx + 4 * R], saved[nx + 4 * R:nx + 5 * R]
        outs = dict(zip(by_dst, saved[nx + 5 * R:]))
        douts = {t: d.contiguous() for t, d in zip(by_dst, douts)}
        dy = [None] * R
        if combine == "+":
            for t, ks in by_dst.items():
                for k in ks:
                    dy[k] = douts[t]
        else:      # the masked identity first: one launch per output width
            for D in sorted({outs[t].shape[1] for t in by_dst}):
                ts = [t for t in by_dst if outs[t].shape[1] == D]
                for t, ds in zip(ts, _fold_grad([(outs[t], douts[t], [ys[k] for k in by_dst[t]]) for t in ts], D)):
                    for k, d in zip(by_dst[t], ds):
                        dy[k] = d
        gparams = [None] * (3 * R)
        roots, walks = {}, {}
        for k, (et, sigma, aggr) in enumerate(members):
            wr, wa, b = params[3 * k:3 * k + 3]
            need = ctx.needs_input_grad[2 + nx + 3 * k:2 + nx + 3 * k + 3]
            dz = act_grad(dy[k], ys[k], sigma)
            gparams[3 * k], gparams[3 * k + 2] = dense_grad_w(dz, x[et[2]], need_w=need[0], need_b=b is not None and need[2])
            if need[1]:
                gparams[3 * k + 1] = dense_grad_w(dz, ms[k], need_b=False)[0]
            roots.setdefault(et[2], []).append(("id", None, dense_grad_x(dz, wr), None, None, None))
            u = dense_grad_x(dz, wa)
            code = aggr_code(aggr)
            if code in (L.MAX, L.MIN):
                walks.setdefault(et[0], []).append(("win", et, u, None, None, ms[k]))
            else:
                walks.setdefault(et[0], []).append(("lin", et, u, None, _inv_count(g, et) if code == L.MEAN else None, None))
        # Δx_S = Σ_{r into S} Δz_r W_root_r (identity terms) + Σ_{r out of S} Aᵀ_r-walk(Δz_r W_agg_r): ONE launch over all types of a width
        per_src = {s: roots.get(s, []) + walks.get(s, []) for s in x_keys if s in roots or s in walks}
        dx = {}
        if any(ctx.needs_input_grad[2:2 + nx]):
            for D in sorted({x[s].shape[1] for s in per_src}):
                dx.update(_src_grad(g, {s: ts for s, ts in per_src.items() if x[s].shape[1] == D}, x, D))
        gx = [dx[k].view(saved[i].shape) if k in dx else torch.zeros_like(saved[i]) for i, k in enumerate(x_keys)]
        return (None, None, *gx, *gparams)


def hetero_conv_ad(layer, g: GNNHeteroGraph, x):
    """differentiable HeteroGraphConv forward of GraphConv / SAGEConv members with σ in identity, relu: gradients w.r.t. every x[node_t]
    and every member's weights and bias (SAGEConv: l.weight, through its [W_root W_agg] column-block views).  Returns {dst_t: y}.
    A layer whose members are ALL GATConv / GATv2Conv is differentiable too (gnnmp/hetero_attn.py: hetero_attn_conv_ad); one that mixes
    attention members with GraphConv / SAGEConv members is refused here (its forward runs, through the composition)."""
    from .hetero_attn import hetero_attn_conv_ad, is_attention_layer
    attn = [is_attention_layer(l) for l in layer.layers]
    if any(attn):
        if not all(attn):
            names = sorted({type(l).__name__ for l in layer.layers})
            raise NotImplementedError(f"hetero_conv_ad: a layer that mixes attention members with GraphConv / SAGEConv members is not "
                                      f"differentiable here (members: {', '.join(names)})")
        return hetero_attn_conv_ad(layer, g, x)
    members = []
    for et, l in zip(layer.etypes, layer.layers):
        if not isinstance(l, _BIPARTITE_LAYERS):
            raise NotImplementedError(f"hetero_conv_ad: {type(l).__name__} does not take a (x_src, x_dst) pair on a bipartite relation "
                                      "(supported: GraphConv, SAGEConv)")
        _act_code(l.sigma)      # ValueError unless identity / relu — before anything runs
        aggr_code(l.aggr)
        members.append((et, l.sigma, l.aggr))
    g._check_num_nodes(x)
    used = [nt for nt in g.ntypes if any(nt in (et[0], et[2]) for et in layer.etypes)]
    params = []
    for et, l in zip(layer.etypes, layer.layers):
        wr, wa = _split_weights(l, x[et[2]].shape[1])
        params += [wr, wa, l.bias]
    out = _HeteroConvFn.apply(g, (tuple(used), tuple(members), layer.aggr), *[x[nt] for nt in used], *params)
    dsts = list(dict.fromkeys(et[2] for et in layer.etypes))
    return dict(zip(dsts, out))
