"""numpy restatements of the ADJOINT of the heterogeneous message passing (tests/hetero_ref.py is the forward), the way NNlib's rrules
state it: ∇gather = scatter(+), ∇scatter(+) = gather, ∇scatter(mean) = gather ./ count, ∇scatter(max | min) = (src .== gather(dst)) .*
gather(Δ); a fold foldl(max | min, terms) hands Δ to every term that equals the result (the project's tie rule, include/gnnmp.h).
Two versions of the same loops:
  dtype = float64   the value reference (bound 1e-5), itself checked against central finite differences of hetero_ref (no GPU needed)
  dtype = float32   the order gnnmp_hetero_propagate_grad_f32 states: per relation the slots of a source row in ORIGINAL edge order, every
                    product rounded (Δ * sd first, then w *), the relations' terms added in table order with the first one copied — the
                    bits the linear and identity modes owe (and, every term being a copy or 0, the winners and masked modes too)
Indices are 0-based here."""
import numpy as np

import hetero_ref as R


# ---- the four modes of one record, and the sum over a source type's records -------------------------------------------------------------
def linear_ref(s, t, n_src, dy, w=None, sd=None, dtype=np.float32):
    """c[j] = Σ_{k: s[k] = j, in edge order} w[k] * (dy[t[k]] * sd[t[k]]); an absent w or sd is 1"""
    dy = np.asarray(dy, dtype)
    c = np.zeros((n_src, dy.shape[1]), dtype)
    for k in range(len(s)):
        m = dy[t[k]]
        if sd is not None:
            m = m * dtype(sd[t[k]])
        if w is not None:
            m = dtype(w[k]) * m
        c[s[k]] = c[s[k]] + m
    return c


def winners_ref(s, t, n_src, x, y, dy, dtype=np.float32):
    """c[j][f] = Σ_{k: s[k] = j} (x[j][f] == y[t[k]][f] ? dy[t[k]][f] : 0) — the comparison on the float32 values the device holds"""
    dy = np.asarray(dy, dtype)
    c = np.zeros((n_src, dy.shape[1]), dtype)
    for k in range(len(s)):
        c[s[k]] = c[s[k]] + np.where(np.asarray(x)[s[k]] == np.asarray(y)[t[k]], dy[t[k]], dtype(0))
    return c


def masked_ref(y, out, dy, dtype=np.float32):
    return np.where(np.asarray(y) == np.asarray(out), np.asarray(dy, dtype), dtype(0))


def sum_ref(terms):
    """c_1 + ... + c_R in table order, the first copied"""
    run = terms[0].copy()
    for c in terms[1:]:
        run = run + c
    return run


# ---- the pullback of hetero_ref (one destination type) -----------------------------------------------------------------------------------
def hetero_grad_ref(rels, n_dst, dout, combine="+", root=None, dtype=np.float64):
    """rels: [(s, t, x_src, w | None, aggr)] as hetero_ref takes them; dout [n_dst, D].  Returns (Δroot | None, [(Δx_src, Δw | None)]) —
    one pair per relation, Δx_src [n_src, D] that relation's share of its source type's gradient."""
    dout = np.asarray(dout, dtype)
    terms = ([] if root is None else [np.asarray(root, dtype)]) + [R.propagate_ref(s, t, n_dst, x, w, a, dtype) for s, t, x, w, a in rels]
    out = R.fold_ref(terms, combine)
    dterms = [dout if combine == "+" else masked_ref(m, out, dout, dtype) for m in terms]
    droot = None if root is None else dterms[0]
    res = []
    for (s, t, x, w, aggr), m, d in zip(rels, terms[len(terms) - len(rels):], dterms[len(terms) - len(rels):]):
        x = np.asarray(x, dtype)
        if aggr in ("max", "min"):
            assert w is None
            res.append((winners_ref(s, t, x.shape[0], x, m, d, dtype), None))
            continue
        sd = None
        if aggr == "mean":
            sd = 1.0 / np.maximum(np.bincount(t, minlength=n_dst), 1).astype(dtype)
        dx = linear_ref(s, t, x.shape[0], d, w, sd, dtype)
        dw = None
        if w is not None:
            dm = d if sd is None else d * sd[:, None]
            dw = np.array([dm[t[k]] @ x[s[k]] for k in range(len(s))], dtype).reshape(len(s))
        res.append((dx, dw))
    return droot, res


# ---- the pullback of hetero_conv_ref -----------------------------------------------------------------------------------------------------
def hetero_conv_grad_ref(layers, graph, num_nodes, x, dout, combine="+", dtype=np.float64):
    """layers: [(edge_t, (W_root, W_agg, bias | None, sigma, aggr))]; dout: {dst_t: Δy}.  Returns ({node_t: Δx}, [(ΔW_root, ΔW_agg, Δb | None)])
    derived from hetero_conv_ref: y_d = foldl(combine, [σ.(x_d W_rootᵀ + m_r W_aggᵀ + b) ...])"""
    x = {k: np.asarray(v, dtype) for k, v in x.items()}
    ys, ms, by_dst = [], [], {}
    for k, (et, (Wr, Wa, b, sigma, aggr)) in enumerate(layers):
        s, t = graph[et]
        ms.append(R.propagate_ref(s, t, num_nodes[et[2]], x[et[0]], None, aggr, dtype))
        ys.append(R.graph_conv_ref(s, t, num_nodes[et[2]], x[et[0]], x[et[2]], Wr, Wa, b, sigma, aggr, dtype))
        by_dst.setdefault(et[2], []).append(k)
    dx = {k: np.zeros_like(v) for k, v in x.items()}
    dparams = [None] * len(layers)
    for d, ks in by_dst.items():
        out = R.fold_ref([ys[k] for k in ks], combine)
        for k in ks:
            et, (Wr, Wa, b, sigma, aggr) = layers[k]
            Wr, Wa = np.asarray(Wr, dtype), np.asarray(Wa, dtype)
            s, t = graph[et]
            dy = np.asarray(dout[d], dtype) if combine == "+" else masked_ref(ys[k], out, dout[d], dtype)
            dz = dy * (ys[k] > 0) if sigma == "relu" else dy
            dparams[k] = (dz.T @ x[et[2]], dz.T @ ms[k], None if b is None else dz.sum(0))
            dx[et[2]] = dx[et[2]] + dz @ Wr
            u = dz @ Wa
            n_src = num_nodes[et[0]]
            if aggr in ("max", "min"):
                dx[et[0]] = dx[et[0]] + winners_ref(s, t, n_src, x[et[0]], ms[k], u, dtype)
            else:
                sd = 1.0 / np.maximum(np.bincount(t, minlength=num_nodes[d]), 1).astype(dtype) if aggr == "mean" else None
                dx[et[0]] = dx[et[0]] + linear_ref(s, t, n_src, u, None, sd, dtype)
    return dx, dparams
