"""Heterograph attention: GATConv and GATv2Conv on a bipartite relation, as members of HeteroGraphConv, forward and training.

Reference: gat_conv / gatv2_conv take (x_src, x_dst) through expand_srcdst (GNNlib/src/layers/conv.jl:112-150, :171-201); HeteroGraphConv
(GraphNeuralNetworks/src/layers/heteroconv.jl:57-86) applies one layer per relation and folds the outputs per destination type.

  gat_conv_pair / gatv2_conv_pair    the layer functions on a (x_src, x_dst) pair — reached through gat_conv / gatv2_conv, which hand a pair
                                     over here and keep a tensor x on their own path.  GAT applies the one dense_x to both sides, GATv2
                                     dense_i to x_dst and dense_j to x_src (as the reference does): both inputs have the layer's `in` width.
  hetero_attn_call                   ONE gnnmp_hetero_attn_f32 launch (csrc/hetero_attn.hip): every destination row finished over all of
                                     its incoming attention relations, the per-relation outputs never written.
  fused_records                      what HeteroGraphConv asks for one destination type: the records of that launch, or None when the type
                                     takes the composition (per member through the pair forwards, then the identity-relation combiner).
  hetero_attn_conv_ad                differentiable HeteroGraphConv of attention members (reached through hetero_conv_ad).

The fused launch is taken when every incoming member is an attention layer with concat = true, no dropout, no dense_e, add_self_loops =
false, σ identity or relu, one common (heads, out), no plan with split rows, a feature row that fits one wave, and knob 22 (KNOB_HETERO)
>= 0; knob 22 < 0 is the A/B baseline.

Outside: TransformerConv and AGNNConv members, edge features and dropout on relations, a fused head mean, chunked hub rows, a one-launch
multi-relation pullback, `batch` of heterographs, Float64.
"""
from __future__ import annotations

import torch

from . import _lib as L
from .graph import check_num_nodes
from .layers import GATConv, _act_code, dense
from .layers_attn import ATTN_GAT, ATTN_GATV2, GATv2Conv, _heads_tail, attn_conv
from .msgpass import _flat
from .utils import expand_srcdst

ATTENTION_LAYERS = (GATConv, GATv2Conv)


def is_attention_layer(l):
    return isinstance(l, ATTENTION_LAYERS)


def _refuse_on_pair(l, e=None, return_alpha=False, exact_order=False):
    """what a (x_src, x_dst) pair does not take, by name, before anything runs"""
    name = type(l).__name__
    if e is not None or getattr(l, "dense_e_weight", None) is not None:
        raise NotImplementedError(f"{name} on a (x_src, x_dst) pair: edge features are not supported on a relation")
    if float(getattr(l, "dropout", 0.0)) > 0.0:
        raise NotImplementedError(f"{name} on a (x_src, x_dst) pair: attention dropout is not supported on a relation")
    if return_alpha or exact_order:
        raise NotImplementedError(f"{name} on a (x_src, x_dst) pair: return_alpha / exact_order are not supported on a relation")
    if l.add_self_loops:
        raise NotImplementedError(f"{name} on a (x_src, x_dst) pair: add_self_loops on a heterograph relation is out of scope "
                                  "(build the layer with add_self_loops=False)")


def _pair(g, x):
    check_num_nodes(g, x)
    xs, xd = expand_srcdst(g, tuple(x))
    xs, xd = _flat(xs), _flat(xd)
    assert xs.shape[1] == xd.shape[1], "x_src and x_dst both have the layer's `in` width (one dense_x / dense_i, dense_j of equal input width)"
    return xs, xd


def gat_conv_pair(l, g, x, e=None, return_alpha=False, exact_order=False):
    """gat_conv(l, g, (x_src, x_dst)) — conv.jl:112-150 with Wxi = dense_x(x_dst), Wxj = dense_x(x_src)"""
    _refuse_on_pair(l, e, return_alpha, exact_order)
    xs, xd = _pair(g, x)
    plan = g.plan(False)
    H, C = l.heads, l.channel[1]
    Ks = dense(xs, l.dense_x_weight)
    Qd = Ks if xd is xs else dense(xd, l.dense_x_weight)
    code, _ = _act_code(l.sigma)
    fuse = bool(l.concat)
    out = torch.empty((plan.n_dst, H * C), dtype=torch.float32, device=xs.device)
    L.check(L.load().gnnmp_gat_conv_f32(plan.handle, L.ptr(Ks), None if Qd is Ks else L.ptr(Qd), L.ptr(l.a_hc), float(l.negative_slope),
                                        L.ptr(l.bias) if (fuse and l.bias is not None) else None, code if fuse else L.ACT_IDENTITY,
                                        L.ptr(out), H, C, L.stream_ptr()))
    return _heads_tail(out, l, plan.n_dst, H, C)


def gatv2_conv_pair(l, g, x, e=None):
    """gatv2_conv(l, g, (x_src, x_dst)) — conv.jl:171-201 with Wxi = dense_i(x_dst), Wxj = dense_j(x_src)"""
    _refuse_on_pair(l, e)
    xs, xd = _pair(g, x)
    plan = g.plan(False)
    H, C = l.heads, l.channel[1]
    code, _ = _act_code(l.sigma)
    fuse = bool(l.concat)
    out = attn_conv(plan, ATTN_GATV2, dense(xs, l.dense_j_weight), Q=dense(xd, l.dense_i_weight, l.dense_i_bias), a=l.a_hc,
                    slope=l.negative_slope, bias=l.bias if (fuse and l.bias is not None) else None,
                    act=code if fuse else L.ACT_IDENTITY, H=H, C=C)
    return _heads_tail(out, l, plan.n_dst, H, C)


# ---------------------------------------------------------------------------------------------------------
# the one-launch multi-relation kernel
# ---------------------------------------------------------------------------------------------------------
def hetero_attn_call(records, H, C):
    """ONE gnnmp_hetero_attn_f32 call.  records: [(out, n_dst, combine code, [(Plan | None, mode, Q | None, K, a | None, bias | None,
    stats | None, slope, act code)])]"""
    dsts = (L.HeteroAttnDst * len(records))()
    keep = []
    p = lambda t: None if t is None else (t.data_ptr() or None)      # noqa: E731
    for d, (out, n_dst, combine, rels) in zip(dsts, records):
        tab = (L.HeteroAttnRel * len(rels))()
        for r, (plan, mode, Q, K, a, bias, stats, slope, act) in zip(tab, rels):
            r.plan = None if plan is None else plan.handle
            r.mode, r.Q, r.K, r.a, r.bias, r.stats, r.negative_slope, r.act = mode, p(Q), p(K), p(a), p(bias), p(stats), float(slope), act
        keep.append(tab)
        d.out, d.n_dst, d.combine, d.n_rel, d.rels = p(out), n_dst, combine, len(rels), tab
    L.check(L.load().gnnmp_hetero_attn_f32(dsts, len(records), H, C, L.stream_ptr()))


def hetero_attn_batches(records, H, C):
    """the records of one (H, C) in as few calls as the relation cap allows, in order"""
    batch, used = [], 0
    for r in records:
        if batch and used + len(r[3]) > L.HETERO_MAX_REL:
            hetero_attn_call(batch, H, C)
            batch, used = [], 0
        batch.append(r)
        used += len(r[3])
    if batch:
        hetero_attn_call(batch, H, C)


def row_fits_wave(H, C):
    """gnnmp_gat_conv_stats_f32's rule for the arrays torch allocates (aligned for any v)"""
    v = 4 if C % 4 == 0 else 2 if C % 2 == 0 else 1
    return H * C // v <= 64


def _describe(l):
    """(attention layer?, concat, dropout, edge features?, add_self_loops, σ, heads, out): all fusable() asks of a member"""
    if not is_attention_layer(l):
        return (False, False, 0.0, False, False, None, 0, 0)
    return (True, bool(l.concat), float(getattr(l, "dropout", 0.0)), getattr(l, "dense_e_weight", None) is not None, bool(l.add_self_loops),
            l.sigma, l.heads, l.channel[1])


def fusable(descs, plans, need_identity=False):
    """may one destination type's members (their _describe records) take the fused launch?  (H, C) if so, else None.  need_identity: the
    caller also needs every σ to be the identity (the training forward, whose pre-activation cotangent is then Δout itself)"""
    if L.knob(L.KNOB_HETERO) < 0 or len(descs) > L.HETERO_MAX_REL:
        return None
    hc = None
    for (attn, concat, dropout, edge, loops, sigma, H, C), p in zip(descs, plans):
        if not attn or not concat or dropout > 0.0 or edge or loops or p.n_long > 0:
            return None
        code, post = _act_code(sigma)
        if post is not None or code not in (L.ACT_IDENTITY, L.ACT_RELU) or (need_identity and code != L.ACT_IDENTITY):
            return None
        if hc is None:
            hc = (H, C)
        if hc != (H, C):
            return None
    return hc if hc is not None and row_fits_wave(*hc) else None


class Projections:
    """dense_x / dense_i / dense_j of a node type's features, each computed once per (weight, bias, node type) however many relations
    share it"""

    def __init__(self, x):
        self.x, self.cache = x, {}

    def __call__(self, W, b, nt):
        key = (W.data_ptr(), None if b is None else b.data_ptr(), nt)
        if key not in self.cache:
            self.cache[key] = dense(_flat(self.x[nt]), W, b)
        return self.cache[key]


def relation_operands(l, et, proj):
    """(mode, Q, K, a) of member l on relation et"""
    if isinstance(l, GATConv):
        return ATTN_GAT, proj(l.dense_x_weight, None, et[2]), proj(l.dense_x_weight, None, et[0]), l.a_hc
    return ATTN_GATV2, proj(l.dense_i_weight, l.dense_i_bias, et[2]), proj(l.dense_j_weight, None, et[0]), l.a_hc


def fused_records(members, plans, proj):
    """the relation records of one destination type for hetero_attn_call and their (H, C), or None: the type takes the composition"""
    hc = fusable([_describe(l) for _, l in members], plans)
    if hc is None:
        return None
    rels = []
    for (et, l), p in zip(members, plans):
        mode, Q, K, a = relation_operands(l, et, proj)
        rels.append((p, mode, Q, K, a, l.bias, None, l.negative_slope, _act_code(l.sigma)[0]))
    return hc, rels


# ---------------------------------------------------------------------------------------------------------
# training
# ---------------------------------------------------------------------------------------------------------
NP = 5      # parameter slots per member: (W | Wi, None | bi, None | Wj, a, bias)


class _HeteroAttnConvFn(torch.autograd.Function):
    """y_d = foldl(aggr, [σ_r.(attn_r(x_src, x_d) .+ b_r) for r into d]) with attn_r the GAT / GATv2 neighbourhood attention of relation r.
    inputs: x by node type, then NP parameter slots per member; outputs: one tensor per destination type.
    A destination type whose members take the fused launch with the fold + and every σ the identity runs gnnmp_hetero_attn_f32 with the
    statistics requested: every relation's pre-activation cotangent is then Δout itself and no per-relation term is kept.  Otherwise the
    per-relation exports keep the terms, and _fold_grad / act_grad apply."""

    @staticmethod
    def forward(ctx, g, spec, *tensors):
        from .backward import _act_code as act_code
        from .hetero import _COMBINE, _combine
        x_keys, members, combine = spec          # members: [(edge_t, kind, H, C, slope, σ, concat)]
        nx = len(x_keys)
        x = {k: _flat(t) for k, t in zip(x_keys, tensors[:nx])}
        params = tensors[nx:]
        lib = L.load()
        f32 = dict(dtype=torch.float32, device=g.device)
        proj = Projections(x)
        R = len(members)
        Qs, Ks, As, stats, ys, by_dst = [None] * R, [None] * R, [None] * R, [None] * R, [None] * R, {}
        for k, (et, kind, H, C, slope, sigma, concat) in enumerate(members):
            W, bi, Wj, a, _ = params[NP * k:NP * k + NP]
            if kind == ATTN_GAT:
                Qs[k], Ks[k] = proj(W, None, et[2]), proj(W, None, et[0])
                As[k] = a.t()[:, :2 * C].contiguous()
            else:
                Qs[k], Ks[k] = proj(W, bi, et[2]), proj(Wj, None, et[0])
                As[k] = a.t().contiguous()
            stats[k] = torch.empty((g.num_nodes[et[2]], H, 2), **f32)
            by_dst.setdefault(et[2], []).append(k)
        out, fused, recs = {}, set(), {}
        for t, ks in by_dst.items():
            hc = None
            if combine == "+":      # (dropout, edge features and self loops were refused before the call)
                hc = fusable([(True, members[k][6], 0.0, False, False, members[k][5], members[k][2], members[k][3]) for k in ks],
                             [g.plan(members[k][0]) for k in ks], need_identity=True)
            if hc is not None:
                out[t] = torch.empty((g.num_nodes[t], hc[0] * hc[1]), **f32)
                rels = [(g.plan(members[k][0]), members[k][1], Qs[k], Ks[k], As[k], params[NP * k + 4], stats[k], members[k][4],
                         L.ACT_IDENTITY) for k in ks]
                recs.setdefault(hc, []).append((out[t], g.num_nodes[t], L.SUM, rels))
                fused.add(t)
        for hc, rs in recs.items():
            hetero_attn_batches(rs, *hc)
        for t, ks in by_dst.items():
            if t in fused:
                continue
            for k in ks:
                et, kind, H, C, slope, sigma, concat = members[k]
                plan, bias = g.plan(et), params[NP * k + 4]
                o = torch.empty((plan.n_dst, H * C), **f32)
                b, act = (bias, act_code(sigma)) if concat else (None, L.ACT_IDENTITY)
                if kind == ATTN_GAT:
                    L.check(lib.gnnmp_gat_conv_stats_f32(plan.handle, L.ptr(Ks[k]), None if Qs[k] is Ks[k] else L.ptr(Qs[k]), L.ptr(As[k]),
                                                         float(slope), L.ptr(b), act, L.ptr(o), L.ptr(stats[k]), H, C, L.stream_ptr()))
                else:
                    L.check(lib.gnnmp_attn_conv_f32(plan.handle, ATTN_GATV2, L.ptr(Qs[k]), L.ptr(Ks[k]), None, L.ptr(As[k]), float(slope), 1.0,
                                                    L.ptr(b), act, L.ptr(o), L.ptr(stats[k]), H, C, L.stream_ptr()))
                if not concat:      # mean over the heads, then σ.(x .+ bias) (conv.jl:143-147)
                    y = torch.empty((plan.n_dst, C), **f32)
                    L.check(lib.gnnmp_head_mean_f32(L.ptr(o), L.ptr(bias), act_code(sigma), L.ptr(y), plan.n_dst, H, C, L.stream_ptr()))
                    o = y
                ys[k] = o
        rest = [t for t in by_dst if t not in fused]
        for D in sorted({ys[by_dst[t][0]].shape[1] for t in rest}):
            out.update(_combine({t: [ys[k] for k in by_dst[t]] for t in rest if ys[by_dst[t][0]].shape[1] == D}, _COMBINE[combine], D))
        ctx.g, ctx.spec, ctx.by_dst, ctx.fused = g, spec, by_dst, fused
        ctx.save_for_backward(*x.values(), *params, *Qs, *Ks, *As, *stats, *ys, *[out[t] for t in by_dst])
        return tuple(out[t] for t in by_dst)

    @staticmethod
    def backward(ctx, *douts):
        from .backward import act_grad, dense_grad_w, dense_grad_x
        from .backward_hetero import _fold_grad
        from .hetero import _combine
        g, by_dst, fused = ctx.g, ctx.by_dst, ctx.fused
        x_keys, members, combine = ctx.spec
        nx, R = len(x_keys), len(members)
        saved = ctx.saved_tensors
        x = dict(zip(x_keys, saved[:nx]))
        o = nx
        params, o = saved[o:o + NP * R], o + NP * R
        Qs, Ks, As, stats, ys = (saved[o + i * R:o + (i + 1) * R] for i in range(5))
        outs = dict(zip(by_dst, saved[o + 5 * R:]))
        douts = {t: d.contiguous() for t, d in zip(by_dst, douts)}
        lib = L.load()
        f32 = dict(dtype=torch.float32, device=g.device)
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
        gparams = [None] * (NP * R)
        terms = {}      # {node_t: [Δx contribution, ...]} in member order, a member's destination side before its source side
        for k, (et, kind, H, C, slope, sigma, concat) in enumerate(members):
            W, bi, Wj, a, bias = params[NP * k:NP * k + NP]
            need = ctx.needs_input_grad[2 + nx + NP * k:2 + nx + NP * k + NP]
            plan, plan_t = g.plan(et), g.plan(et, transposed=True)
            n_dst, n_src = plan.n_dst, plan.n_src
            xs, xd = x[et[0]], x[et[2]]
            dz = dy[k] if et[2] in fused else act_grad(dy[k], ys[k], sigma)
            if bias is not None and need[4]:
                gparams[NP * k + 4] = dense_grad_w(dz, dz, need_w=False, need_b=True)[1]
            if not concat:                       # pullback of mean(x, dims = 2): every head receives Δ / H
                dzh = torch.empty((n_dst, H * C), **f32)
                L.check(lib.gnnmp_head_mean_grad_f32(L.ptr(dz), L.ptr(dzh), n_dst, H, C, L.stream_ptr()))
                dz = dzh
            line = torch.empty((n_dst, H, 4), **f32)
            dK = torch.empty((n_src, H * C), **f32)
            if kind == ATTN_GAT:
                same = Qs[k].data_ptr() == Ks[k].data_ptr() and n_src == n_dst      # one projection serves both sides
                dQ = None if same else torch.empty((n_dst, H * C), **f32)
                dsd, dss = torch.empty((n_dst, H), **f32), torch.empty((n_src, H), **f32)
                da = torch.empty((H, 2 * C), **f32)
                L.check(lib.gnnmp_gat_conv_grad_f32(plan.handle, plan_t.handle, L.ptr(Ks[k]), None if same else L.ptr(Qs[k]), L.ptr(As[k]),
                                                    float(slope), L.ptr(stats[k]), L.ptr(dz), L.ptr(line), L.ptr(dsd), L.ptr(dss), L.ptr(dK),
                                                    L.ptr(dQ), L.ptr(da), H, C, L.stream_ptr()))
                if need[0]:
                    dW = dense_grad_w(dK, xs, need_b=False)[0]
                    if dQ is not None:
                        dWq = dense_grad_w(dQ, xd, need_b=False)[0]
                        L.check(lib.gnnmp_add_f32(L.ptr(dWq), L.ptr(dW), L.ptr(dW), dW.numel(), L.stream_ptr()))
                    gparams[NP * k] = dW
                if dQ is not None:
                    terms.setdefault(et[2], []).append(dense_grad_x(dQ, W))
                terms.setdefault(et[0], []).append(dense_grad_x(dK, W))
            else:
                dQ, dA = torch.empty((n_dst, H * C), **f32), torch.empty((n_dst, H * C), **f32)
                da = torch.empty((H, C), **f32)
                L.check(lib.gnnmp_attn_conv_grad_f32(plan.handle, plan_t.handle, ATTN_GATV2, L.ptr(Qs[k]), L.ptr(Ks[k]), None, L.ptr(As[k]),
                                                     float(slope), 1.0, L.ptr(stats[k]), L.ptr(dz), L.ptr(line), L.ptr(dQ), L.ptr(dK), None,
                                                     L.ptr(dA), L.ptr(da), H, C, L.stream_ptr()))
                gparams[NP * k], gparams[NP * k + 1] = dense_grad_w(dQ, xd, need_w=need[0], need_b=bi is not None and need[1])
                if need[2]:
                    gparams[NP * k + 2] = dense_grad_w(dK, xs, need_b=False)[0]
                terms.setdefault(et[2], []).append(dense_grad_x(dQ, W))
                terms.setdefault(et[0], []).append(dense_grad_x(dK, Wj))
            if need[3]:
                gparams[NP * k + 3] = da.t()
        # Δx of one node type: its contributions summed in that fixed order by the identity relations of gnnmp_hetero_propagate_f32
        dx = {}
        if any(ctx.needs_input_grad[2:2 + nx]):
            for D in sorted({ts[0].shape[1] for ts in terms.values()}):
                dx.update(_combine({s: ts for s, ts in terms.items() if ts[0].shape[1] == D}, L.SUM, D))
        gx = [dx[k].view(saved[i].shape) if k in dx else torch.zeros_like(saved[i]) for i, k in enumerate(x_keys)]
        return (None, None, *gx, *gparams)


def hetero_attn_conv_ad(layer, g, x):
    """differentiable HeteroGraphConv forward of GATConv / GATv2Conv members (σ identity or relu, concat true or false): gradients w.r.t.
    every x[node_t] and dense_x_weight / a / bias (GAT), dense_i_weight / dense_i_bias / dense_j_weight / a / bias (GATv2).
    Returns {dst_t: y}."""
    from .backward import _act_code as act_code
    members, params = [], []
    for et, l in zip(layer.etypes, layer.layers):
        _refuse_on_pair(l)
        act_code(l.sigma)      # ValueError unless identity / relu — before anything runs
        if isinstance(l, GATConv):
            kind, ps = ATTN_GAT, [l.dense_x_weight, None, None, l.a, l.bias]
        else:
            kind, ps = ATTN_GATV2, [l.dense_i_weight, l.dense_i_bias, l.dense_j_weight, l.a, l.bias]
        members.append((et, kind, l.heads, l.channel[1], float(l.negative_slope), l.sigma, bool(l.concat)))
        params += ps
    g._check_num_nodes(x)
    used = [nt for nt in g.ntypes if any(nt in (et[0], et[2]) for et in layer.etypes)]
    for et, l in zip(layer.etypes, layer.layers):
        assert x[et[0]].shape[1] == l.channel[0] and x[et[2]].shape[1] == l.channel[0], \
            f"relation {et}: x_src and x_dst both have the layer's `in` width {l.channel[0]}"
    out = _HeteroAttnConvFn.apply(g, (tuple(used), tuple(members), layer.aggr), *[x[nt] for nt in used], *params)
    dsts = list(dict.fromkeys(et[2] for et in layer.etypes))
    return dict(zip(dsts, out))
