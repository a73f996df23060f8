"""Float64 numpy restatement of heterograph attention: the semantics of gnnmp_hetero_attn_f32 (include/gnnmp.h), the GATConv / GATv2Conv
layer forwards on a relation (gat_conv / gatv2_conv through expand_srcdst, GNNlib/src/layers/conv.jl:112-214), HeteroGraphConv over them
(GraphNeuralNetworks/src/layers/heteroconv.jl:57-86), and their gradients rule by rule.  Indices are 0-based here.

  attn_rel(s, t, n_dst, Q, K, a, mode, slope, H, C)              (o [n_dst, H*C], stats [n_dst, H, 2] = (m_i, den_i))
  hetero_attn(rels, n_dst, combine, H, C)                        (out, [stats per relation]) — the export
  attn_rel_grad(..., do)                                         (dQ, dK, da) — the pullback of attn_rel's o
  layer_forward(p, s, t, n_dst, xs, xd)                          a member's output on its relation; p: a dict, see gat_params / gatv2_params
  layer_grad(p, s, t, n_dst, xs, xd, dy)                         (dxs, dxd, {parameter name: gradient})
  conv_forward(members, coo, num, x, combine)                    {dst_t: y}
  conv_grad(members, coo, num, x, dout, combine)                 ({node_t: dx}, [{parameter name: gradient} per member])

Rules the gradients follow (the project's, gnnmp/backward_hetero.py): relu' = (y > 0); in a fold of max / min EVERY term that ties with the
result receives the cotangent."""
import numpy as np

GAT, GATV2 = 0, 1
f64 = np.float64


def lrelu(z, slope):
    return np.where(z > 0, z, slope * z)


def _logits(s, t, Q, K, a, mode, slope, H, C):
    Q, K, a = Q.reshape(-1, H, C), K.reshape(-1, H, C), np.asarray(a, f64)
    if mode == GAT:          # a [H][2C], target half first
        return lrelu((a[None, :, :C] * Q).sum(-1)[t] + (a[None, :, C:] * K).sum(-1)[s], slope)
    return (a[None] * lrelu(Q[t] + K[s], slope)).sum(-1)


def _softmax(l, t, n_dst, H):
    m = np.full((n_dst, H), -np.inf)
    np.maximum.at(m, t, l)
    p = np.exp(l - m[t])
    den = np.zeros((n_dst, H))
    np.add.at(den, t, p)
    return p / den[t], m, den


def attn_rel(s, t, n_dst, Q, K, a, mode, slope, H, C):
    s, t = np.asarray(s, np.int64), np.asarray(t, np.int64)
    Q, K = np.asarray(Q, f64), np.asarray(K, f64)
    alpha, m, den = _softmax(_logits(s, t, Q, K, a, mode, slope, H, C), t, n_dst, H)
    o = np.zeros((n_dst, H, C))
    np.add.at(o, t, alpha[..., None] * K.reshape(-1, H, C)[s])
    return o.reshape(n_dst, H * C), np.stack([m, den], -1)


def act(y, sigma):
    return np.maximum(y, 0.0) if sigma in ("relu", 1) else y


def fold(terms, combine):
    out = terms[0]
    for term in terms[1:]:
        out = out + term if combine == "+" else (np.maximum(out, term) if combine == "max" else np.minimum(out, term))
    return out


def hetero_attn(rels, n_dst, combine, H, C):
    """rels: [dict(s, t, mode, Q, K, a, bias, slope, act)] — s None: an identity relation, row i of K as it is"""
    terms, stats = [], []
    for r in rels:
        if r.get("s") is None:
            terms.append(np.asarray(r["K"], f64).reshape(n_dst, H * C))
            stats.append(None)
            continue
        o, st = attn_rel(r["s"], r["t"], n_dst, r["Q"], r["K"], r["a"], r["mode"], r["slope"], H, C)
        if r.get("bias") is not None:
            o = o + np.asarray(r["bias"], f64)[None]
        terms.append(act(o, r.get("act")))
        stats.append(st)
    return fold(terms, combine), stats


def attn_rel_grad(s, t, n_dst, Q, K, a, mode, slope, H, C, do):
    s, t = np.asarray(s, np.int64), np.asarray(t, np.int64)
    Q, K, a = np.asarray(Q, f64).reshape(-1, H, C), np.asarray(K, f64).reshape(-1, H, C), np.asarray(a, f64)
    do = np.asarray(do, f64).reshape(n_dst, H, C)
    alpha, _, _ = _softmax(_logits(s, t, Q, K, a, mode, slope, H, C), t, n_dst, H)
    g = (do[t] * K[s]).sum(-1)                       # Δα
    D = np.zeros((n_dst, H))
    np.add.at(D, t, alpha * g)
    dl = alpha * (g - D[t])                          # the softmax pullback
    dQ, dK = np.zeros_like(Q), np.zeros_like(K)
    np.add.at(dK, s, alpha[..., None] * do[t])       # the value
    if mode == GAT:
        pre = (a[None, :, :C] * Q).sum(-1)[t] + (a[None, :, C:] * K).sum(-1)[s]
        dpre = dl * np.where(pre > 0, 1.0, slope)
        dsd, dss = np.zeros((Q.shape[0], H)), np.zeros((K.shape[0], H))
        np.add.at(dsd, t, dpre)
        np.add.at(dss, s, dpre)
        dQ += dsd[..., None] * a[None, :, :C]
        dK += dss[..., None] * a[None, :, C:]
        da = np.concatenate([(dsd[..., None] * Q).sum(0), (dss[..., None] * K).sum(0)], 1)
    else:
        z = Q[t] + K[s]
        dz = dl[..., None] * a[None] * np.where(z > 0, 1.0, slope)
        np.add.at(dQ, t, dz)
        np.add.at(dK, s, dz)
        da = (dl[..., None] * lrelu(z, slope)).sum(0)
    return dQ.reshape(-1, H * C), dK.reshape(-1, H * C), da


# ---- the layers ---------------------------------------------------------------------------------------------------------------------
def gat_params(W, a, bias, H, sigma=None, concat=True, slope=0.2):
    """W [H*C, in]; a in the layer's Julia shape (2C, H); bias [H*C] (concat) or [C], or None"""
    return dict(kind=GAT, W=np.asarray(W, f64), a=np.asarray(a, f64), bias=None if bias is None else np.asarray(bias, f64), H=H,
                C=W.shape[0] // H, sigma=sigma, concat=concat, slope=slope)


def gatv2_params(Wi, bi, Wj, a, bias, H, sigma=None, concat=True, slope=0.2):
    """Wi, Wj [H*C, in]; bi [H*C] or None; a in the layer's Julia shape (C, H)"""
    return dict(kind=GATV2, Wi=np.asarray(Wi, f64), bi=None if bi is None else np.asarray(bi, f64), Wj=np.asarray(Wj, f64),
                a=np.asarray(a, f64), bias=None if bias is None else np.asarray(bias, f64), H=H, C=Wi.shape[0] // H, sigma=sigma,
                concat=concat, slope=slope)


def _operands(p, xs, xd):
    xs, xd = np.asarray(xs, f64), np.asarray(xd, f64)
    if p["kind"] == GAT:      # the one dense_x on both sides
        return xd @ p["W"].T, xs @ p["W"].T, p["a"].T
    return xd @ p["Wi"].T + (0 if p["bi"] is None else p["bi"][None]), xs @ p["Wj"].T, p["a"].T


def _tail(p, o, n_dst):
    """concat: σ.(o .+ b); else mean over the heads first (conv.jl:143-147).  Returns the pre-activation"""
    H, C = p["H"], p["C"]
    z = o if p["concat"] else o.reshape(n_dst, H, C).mean(1)
    return z + (0 if p["bias"] is None else p["bias"][None])


def layer_forward(p, s, t, n_dst, xs, xd):
    Q, K, a = _operands(p, xs, xd)
    o, _ = attn_rel(s, t, n_dst, Q, K, a, p["kind"], p["slope"], p["H"], p["C"])
    return act(_tail(p, o, n_dst), p["sigma"])


def layer_grad(p, s, t, n_dst, xs, xd, dy):
    H, C = p["H"], p["C"]
    xs, xd = np.asarray(xs, f64), np.asarray(xd, f64)
    Q, K, a = _operands(p, xs, xd)
    o, _ = attn_rel(s, t, n_dst, Q, K, a, p["kind"], p["slope"], H, C)
    y = act(_tail(p, o, n_dst), p["sigma"])
    dz = np.asarray(dy, f64) * (y > 0) if p["sigma"] == "relu" else np.asarray(dy, f64)
    grads = {"bias": None if p["bias"] is None else dz.sum(0)}
    do = dz if p["concat"] else np.repeat(dz[:, None, :] / H, H, axis=1).reshape(n_dst, H * C)
    dQ, dK, da = attn_rel_grad(s, t, n_dst, Q, K, a, p["kind"], p["slope"], H, C, do)
    grads["a"] = da.T
    if p["kind"] == GAT:
        grads["W"] = dQ.T @ xd + dK.T @ xs
        return dK @ p["W"], dQ @ p["W"], grads
    grads["Wi"], grads["Wj"] = dQ.T @ xd, dK.T @ xs
    grads["bi"] = None if p["bi"] is None else dQ.sum(0)
    return dK @ p["Wj"], dQ @ p["Wi"], grads


# ---- HeteroGraphConv ----------------------------------------------------------------------------------------------------------------
def conv_forward(members, coo, num, x, combine):
    """members: [(edge_t, params)]; coo: {edge_t: (s, t)}; num: {node_t: n}; x: {node_t: [n, in]}"""
    terms = {}
    for et, p in members:
        terms.setdefault(et[2], []).append(layer_forward(p, *coo[et], num[et[2]], x[et[0]], x[et[2]]))
    return {k: fold(v, combine) for k, v in terms.items()}


def conv_grad(members, coo, num, x, dout, combine):
    ys, by_dst = [], {}
    for k, (et, p) in enumerate(members):
        ys.append(layer_forward(p, *coo[et], num[et[2]], x[et[0]], x[et[2]]))
        by_dst.setdefault(et[2], []).append(k)
    dx = {k: np.zeros_like(np.asarray(v, f64)) for k, v in x.items()}
    grads = [None] * len(members)
    for dst, ks in by_dst.items():
        out = fold([ys[k] for k in ks], combine)
        for k in ks:
            et, p = members[k]
            d = np.asarray(dout[dst], f64)
            if combine != "+" and len(ks) > 1:
                d = d * (ys[k] == out)
            dxs, dxd, grads[k] = layer_grad(p, *coo[et], num[dst], x[et[0]], x[dst], d)
            dx[et[0]] += dxs
            dx[dst] += dxd
    return dx, grads
