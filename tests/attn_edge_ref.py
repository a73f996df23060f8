"""Float64 numpy restatement of gatv2_conv and transformer_conv WITH edge features (GNNlib/src/layers/conv.jl:171-214 and :553-629):
gather, per-edge message, neighbourhood softmax, scatter-add in edge order, head mean, root weight, skip connection — and their
gradients, written out analytically (tests/test_attn_edge_ref.py holds them against central finite differences).

Indices are 0-based.  Node arrays are [n][H][C] inside the attention core and [n][H*C] outside, edge arrays [E][...] in edge order.
Weights have the Flux shape [out, in] (y = x W' + b); `a` has the Julia shape (C, H)."""
import numpy as np

f64 = np.float64


# ---- the attention cores ---------------------------------------------------------------------------------------------------------
def scatter_add(vals, idx, n):
    out = np.zeros((n,) + vals.shape[1:], f64)
    np.add.at(out, idx, vals)
    return out


def softmax_neighbors(t, n, l):
    """softmax_edge_neighbors (utils.jl:84-97) of l [E][H] over the edges that share a target"""
    m = np.full((n,) + l.shape[1:], -np.inf)
    np.maximum.at(m, t, l)
    ex = np.exp(l - m[t])
    den = scatter_add(ex, t, n)
    return ex / den[t], m, den


def core(mode, s, t, n, Q, K, V, F, a_hc, slope, scale):
    """(o [n][H][C], cache).  gatv2: z = Q_i + K_j + F_k, l = Σ_c a_c lrelu(z_c), val = K_j;  dot: l = Q_i . (K_j + F_k) / scale,
    val = V_j + F_k"""
    if mode == "gatv2":
        z = Q[t] + K[s] + F
        lr = np.where(z > 0, z, slope * z)
        l = (a_hc[None] * lr).sum(-1)
        val = K[s]
        extra = (z, lr)
    else:
        key = K[s] + F
        l = (Q[t] * key).sum(-1) / scale
        val = V[s] + F
        extra = (key,)
    al, m, den = softmax_neighbors(t, n, l)
    o = scatter_add(al[..., None] * val, t, n)
    return o, dict(al=al, val=val, extra=extra, m=m, den=den, l=l)


def core_grad(mode, s, t, n, Q, K, V, F, a_hc, slope, scale, cache, do):
    """the pullback of core for do = dL/do [n][H][C]: dict of dQ, dK, dV (dot), dF, da [H][C] (gatv2), line D [n][H]"""
    al, val = cache["al"], cache["val"]
    g = (do[t] * val).sum(-1)
    D = scatter_add(al * g, t, n)
    dl = al * (g - D[t])
    dval = al[..., None] * do[t]
    if mode == "gatv2":
        z, lr = cache["extra"]
        dz = dl[..., None] * a_hc[None] * np.where(z > 0, 1.0, slope)
        return dict(dQ=scatter_add(dz, t, n), dK=scatter_add(dz, s, n) + scatter_add(dval, s, n), dF=dz,
                    dA=scatter_add(dl[..., None] * lr, t, n), da=(dl[..., None] * lr).sum(0), D=D)
    (key,) = cache["extra"]
    dkey = dl[..., None] * Q[t] / scale
    return dict(dQ=scatter_add(dl[..., None] * key / scale, t, n), dK=scatter_add(dkey, s, n), dV=scatter_add(dval, s, n),
                dF=dkey + dval, D=D)


# ---- the layers ------------------------------------------------------------------------------------------------------------------
def lin(x, W, b=None):
    y = x @ W.T
    return y if b is None else y + b[None, :]


def _act(name, z):
    return np.where(z < 0, 0.0, z) if name == "relu" else z


def _as64(p):
    return {k: (np.asarray(v, f64) if isinstance(v, np.ndarray) else v) for k, v in p.items()}


def gatv2_layer(s, t, n, x, e, p):
    """p: Wi, bi | None, Wj, We | None (None: no edge features), a (C, H), bias | None, sigma (None | 'relu'), H, concat, slope.
    Returns (y, cache)"""
    p = _as64(p)
    x = np.asarray(x, f64)
    H = p["H"]
    C = p["Wi"].shape[0] // H
    Q, K = lin(x, p["Wi"], p["bi"]).reshape(n, H, C), lin(x, p["Wj"]).reshape(n, H, C)
    F = lin(np.asarray(e, f64), p["We"]).reshape(-1, H, C) if p["We"] is not None else np.zeros((len(s), H, C))
    a_hc = p["a"].T
    o, cache = core("gatv2", s, t, n, Q, K, None, F, a_hc, p["slope"], 1.0)
    pre = o.reshape(n, H * C) if p["concat"] else o.mean(1)
    if p["bias"] is not None:
        pre = pre + p["bias"][None, :]
    cache.update(Q=Q, K=K, F=F, a_hc=a_hc, pre=pre, C=C, o=o)
    return _act(p["sigma"], pre), cache


def gatv2_grad(s, t, n, x, e, p, r):
    """gradients of Σ y ⊙ r: dict with dx, de, dWi, dbi, dWj, dWe, da (C, H), dbias (None where the operand is None)"""
    p = _as64(p)
    x, r = np.asarray(x, f64), np.asarray(r, f64)
    _, c = gatv2_layer(s, t, n, x, e, p)
    H, C = p["H"], c["C"]
    dz = r * (c["pre"] > 0) if p["sigma"] == "relu" else r
    do = dz.reshape(n, H, C) if p["concat"] else np.repeat(dz[:, None, :] / H, H, axis=1)
    gr = core_grad("gatv2", s, t, n, c["Q"], c["K"], None, c["F"], c["a_hc"], p["slope"], 1.0, c, do)
    dQ, dK, dF = gr["dQ"].reshape(n, -1), gr["dK"].reshape(n, -1), gr["dF"].reshape(len(s), -1)
    out = dict(dx=dQ @ p["Wi"] + dK @ p["Wj"], dWi=dQ.T @ x, dbi=None if p["bi"] is None else dQ.sum(0), dWj=dK.T @ x,
               da=gr["da"].T, dbias=None if p["bias"] is None else dz.sum(0), de=None, dWe=None, core=gr)
    if p["We"] is not None:
        out["de"], out["dWe"] = dF @ p["We"], dF.T @ np.asarray(e, f64)
    return out


def transformer_layer(s, t, n, x, e, p):
    """p: W1 | None, b1, W2, b2, W3, b3, W4, b4, W6 | None, b6, H, concat, skip.  Returns (h, cache)"""
    p = _as64(p)
    x = np.asarray(x, f64)
    H = p["H"]
    C = p["W2"].shape[0] // H
    V, Q, K = (lin(x, p[w], p[b]).reshape(n, H, C) for w, b in (("W2", "b2"), ("W3", "b3"), ("W4", "b4")))
    F = lin(np.asarray(e, f64), p["W6"], p["b6"]).reshape(-1, H, C) if p["W6"] is not None else np.zeros((len(s), H, C))
    scale = float(np.sqrt(np.float32(C)))                # Float32(√out)
    o, cache = core("dot", s, t, n, Q, K, V, F, None, 0.0, scale)
    h = o.reshape(n, H * C) if p["concat"] else o.mean(1)
    if p["W1"] is not None:
        h = h + lin(x, p["W1"], p["b1"])
    if p["skip"]:
        assert h.shape[1] == x.shape[1]
        h = h + x
    cache.update(Q=Q, K=K, V=V, F=F, C=C, scale=scale, o=o)
    return h, cache


def transformer_grad(s, t, n, x, e, p, r):
    """gradients of Σ h ⊙ r: dict with dx, de, dW1 .. dW4, dW6, db1 .. db4, db6 (None where the operand is None)"""
    p = _as64(p)
    x, r = np.asarray(x, f64), np.asarray(r, f64)
    _, c = transformer_layer(s, t, n, x, e, p)
    H, C = p["H"], c["C"]
    do = r.reshape(n, H, C) if p["concat"] else np.repeat(r[:, None, :] / H, H, axis=1)
    gr = core_grad("dot", s, t, n, c["Q"], c["K"], c["V"], c["F"], None, 0.0, c["scale"], c, do)
    dQ, dK, dV, dF = (gr[k].reshape(gr[k].shape[0], -1) for k in ("dQ", "dK", "dV", "dF"))
    out = dict(dx=dV @ p["W2"] + dQ @ p["W3"] + dK @ p["W4"], dW2=dV.T @ x, dW3=dQ.T @ x, dW4=dK.T @ x, core=gr)
    for k, d in (("2", dV), ("3", dQ), ("4", dK)):
        out["db" + k] = None if p["b" + k] is None else d.sum(0)
    out["dW1"] = out["db1"] = out["de"] = out["dW6"] = out["db6"] = None
    if p["W1"] is not None:
        out["dW1"], out["dx"] = r.T @ x, out["dx"] + r @ p["W1"]
        out["db1"] = None if p["b1"] is None else r.sum(0)
    if p["skip"]:
        out["dx"] = out["dx"] + r
    if p["W6"] is not None:
        out["de"], out["dW6"] = dF @ p["W6"], dF.T @ np.asarray(e, f64)
        out["db6"] = None if p["b6"] is None else dF.sum(0)
    return out


# ---- the cases -------------------------------------------------------------------------------------------------------------------
N_NODES, HUB, N_DUP = 48, 600, 20
NO_IN, ONE_IN, NINE_IN, HUB_IN, HUB_OUT = 0, 1, 2, 3, 4


def graph():
    """48 nodes, SHUFFLED edge list (plan slot != edge position): node 0 without in-edges, node 1 with one, node 2 with nine (a full
    batch of the kernels plus a tail), node 3 with 600 in-edges and node 4 with 600 out-edges (above any split threshold of a plan),
    twenty (s, t) pairs listed twice.  Returns (s, t) 0-based int64"""
    rng = np.random.default_rng(48)
    lo = 5
    s = [rng.integers(lo, N_NODES, HUB), np.full(HUB, HUB_OUT), [7], rng.integers(lo, N_NODES, 9), rng.integers(lo, N_NODES, 150), [0, 0, 0]]
    t = [np.full(HUB, HUB_IN), rng.integers(lo, N_NODES, HUB), [ONE_IN], np.full(9, NINE_IN), rng.integers(4, N_NODES, 150), [9, 17, 30]]
    s, t = np.concatenate(s).astype(np.int64), np.concatenate(t).astype(np.int64)
    dup = 2 * HUB + 10 + rng.choice(150, N_DUP, replace=False)
    s, t = np.concatenate([s, s[dup]]), np.concatenate([t, t[dup]])
    perm = rng.permutation(len(s))
    return s[perm], t[perm]


def assert_graph(s, t):
    indeg, outdeg = np.bincount(t, minlength=N_NODES), np.bincount(s, minlength=N_NODES)
    assert indeg[NO_IN] == 0 and indeg[ONE_IN] == 1 and indeg[NINE_IN] == 9 and indeg[HUB_IN] == HUB and outdeg[HUB_OUT] >= HUB
    pairs, counts = np.unique(np.stack([s, t]), axis=1, return_counts=True)
    assert (counts >= 2).sum() >= N_DUP
    assert not np.array_equal(np.argsort(t, kind="stable"), np.arange(len(t)))      # the list is not sorted by destination


def glorot(rng, rows, cols):
    lim = np.sqrt(6.0 / (rows + cols))
    return rng.uniform(-lim, lim, (rows, cols)).astype(np.float32)


def gatv2_params(rng, cin, ein, H, C, concat, sigma="relu", edge=True):
    return dict(Wi=glorot(rng, H * C, cin), bi=(0.1 * rng.standard_normal(H * C)).astype(np.float32), Wj=glorot(rng, H * C, cin),
                We=glorot(rng, H * C, ein) if edge else None, a=glorot(rng, C, H),
                bias=(0.1 * rng.standard_normal(H * C if concat else C)).astype(np.float32), sigma=sigma, H=H, concat=concat, slope=0.2)


def transformer_params(rng, cin, ein, H, C, concat, root, skip, edge=True):
    om = C * (H if concat else 1)
    bias = lambda k: (0.1 * rng.standard_normal(k)).astype(np.float32)      # noqa: E731
    p = dict(W1=glorot(rng, om, cin) if root else None, b1=bias(om) if root else None, H=H, concat=concat, skip=skip)
    for k in "234":
        p["W" + k], p["b" + k] = glorot(rng, H * C, cin), bias(H * C)
    p["W6"], p["b6"] = (glorot(rng, H * C, ein), bias(H * C)) if edge else (None, None)
    return p


def rel(a, b):
    return np.linalg.norm(np.asarray(a, f64) - b) / max(np.linalg.norm(b), 1e-30)
