"""numpy restatements of the reference's heterogeneous message passing that the heterograph tests compare against: per relation
gather -> message -> scatter (GNNlib/src/msgpass.jl:71-79 on the relation's bipartite subgraph, rows = num_nodes[dst_t]:151-156), then
`foldl(aggr, outs)` per destination type (GraphNeuralNetworks/src/layers/heteroconv.jl:68-78).  Two versions of the same loop:
  dtype = float64   the value reference (bound 1e-5)
  dtype = float32   adds in ORIGINAL edge order, every product rounded, folds in relation order: the bits the kernel owes
Indices are 0-based here."""
import numpy as np

IDENT = {"+": 0.0, "mean": 0.0, "max": -np.inf, "min": np.inf}


def propagate_ref(s, t, n_dst, x, w=None, aggr="+", dtype=np.float32):
    """aggregate_neighbors(aggr, w_mul_xj | copy_xj): out[i] = aggr over the edges k with t[k] = i, in edge order, of w[k] * x[s[k]];
    an empty row keeps the identity (NNlib.scatter), mean = sum / count"""
    x = np.asarray(x, dtype)
    out = np.full((n_dst, x.shape[1]), IDENT[aggr], dtype)
    cnt = np.zeros(n_dst, np.int64)
    for k in range(len(s)):
        m = x[s[k]] if w is None else dtype(w[k]) * x[s[k]]
        i = t[k]
        cnt[i] += 1
        if aggr == "max":
            out[i] = np.maximum(out[i], m)
        elif aggr == "min":
            out[i] = np.minimum(out[i], m)
        else:
            out[i] = out[i] + m
    if aggr == "mean":
        nz = cnt > 0
        out[nz] = out[nz] / cnt[nz].astype(dtype)[:, None]
    return out


def fold_ref(terms, combine="+"):
    """foldl(combine, terms): ((m_1 ⊕ m_2) ⊕ m_3) ..., in the terms' own dtype"""
    run = terms[0].copy()
    with np.errstate(invalid="ignore"):          # -Inf + Inf of rows that are empty under max AND min
        for m in terms[1:]:
            run = run + m if combine == "+" else (np.maximum(run, m) if combine == "max" else np.minimum(run, m))
    return run


def hetero_ref(rels, n_dst, combine="+", dtype=np.float32, root=None):
    """one destination type.  rels: [(s, t, x_src, w | None, aggr)] in table order; root: [n_dst, D] entering the fold first"""
    terms = [] if root is None else [np.asarray(root, dtype)]
    terms += [propagate_ref(s, t, n_dst, x, w, aggr, dtype) for s, t, x, w, aggr in rels]
    return fold_ref(terms, combine)


def graph_conv_ref(s, t, n_dst, x_src, x_dst, W_root, W_agg, bias=None, sigma=None, aggr="+", dtype=np.float64):
    """graph_conv / sage_conv on a bipartite relation (GNNlib/src/layers/conv.jl:102-108, 277-283): σ.(W_root x_i + W_agg aggr_j x_j + b)"""
    m = propagate_ref(s, t, n_dst, x_src, None, aggr, dtype)
    with np.errstate(invalid="ignore"):          # ∓Inf rows of max / min over no edges: Inf or NaN after the product
        y = np.asarray(x_dst, dtype) @ np.asarray(W_root, dtype).T + m @ np.asarray(W_agg, dtype).T
    if bias is not None:
        y = y + np.asarray(bias, dtype)[None, :]
    return np.maximum(y, 0) if sigma == "relu" else y


def hetero_conv_ref(layers, graph, num_nodes, x, combine="+", dtype=np.float64):
    """HeteroGraphConv.  layers: [(edge_t, (W_root, W_agg, bias, sigma, aggr))]; graph: {edge_t: (s, t)}; returns {dst_t: array}"""
    outs = {}
    for et, (Wr, Wa, b, sigma, aggr) in layers:
        s, t = graph[et]
        outs.setdefault(et[2], []).append(graph_conv_ref(s, t, num_nodes[et[2]], x[et[0]], x[et[2]], Wr, Wa, b, sigma, aggr, dtype))
    return {d: fold_ref(ys, combine) for d, ys in outs.items()}
