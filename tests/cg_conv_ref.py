"""numpy references of tests/test_cg_conv_ad.py — TEST INFRASTRUCTURE ONLY.

  * compose / grad64: the reference's own composition of CGConv (GNNlib/src/layers/conv.jl:304-333: the per-edge vcat(xi, xj, e), the two
    Dense on E rows, sigmoid .* act, the scatter(+), the residual) restated in float64, and its pullback written by hand.
  * split_fs / rows / rows_grad / layer: the formulation of include/gnnmp.h (fs_i, fs_j, fs_e planar; f_k and s_k summed in the forward's
    order; dfs_i, dfs_j, dfs_e; then the dense adjoints) in the dtype of its operands, every fold a sequential loop in edge order.
  * the operands of every GPU case, with seeds picked by a search on the CPU (find_seed) for inputs on which float32 stays within 2e-6 of
    float64 and, for relu, away from the kink.
Edge indices are 0-based here."""
import numpy as np

f32, f64 = np.float32, np.float64
ACTS = ("identity", "relu", "softplus", "tanh")
ACT_CODE = {"identity": 0, "relu": 1, "softplus": 2, "tanh": 3}
MARGIN = 20         # relu's kink is at least this many times farther away than float32 is from float64 (tests/test_edge_conv_ad.py)
COND = 2e-6         # a fifth of the project's 1e-5 bar


def sigmoid(v):
    """NNlib.sigmoid: t = exp(-abs(x)); ifelse(x >= 0, inv(1 + t), t / (1 + t)), in v's dtype"""
    one = v.dtype.type(1)
    t = np.exp(-np.abs(v))
    return np.where(v >= 0, one / (one + t), t / (one + t))


def dsigmoid(v):
    return sigmoid(v) * sigmoid(-v)


def act(v, name):
    if name == "relu":
        return np.where(v < 0, v.dtype.type(0), v)
    if name == "softplus":
        return np.log1p(np.exp(-np.abs(v))) + np.where(v < 0, v.dtype.type(0), v)      # NNlib.softplus
    if name == "tanh":
        return np.tanh(v)
    return v


def dact(v, name):
    one = v.dtype.type(1)
    if name == "relu":
        return np.where(v > 0, one, v.dtype.type(0))       # 0 at 0
    if name == "softplus":
        return sigmoid(v)
    if name == "tanh":
        a = np.tanh(v)
        return (one - a) * (one + a)
    return np.ones_like(v)


# ---- the reference's composition, float64 -----------------------------------------------------------------------------------------
def compose(s, t, n, x, e, Wf, Ws, bf, bs, name, residual):
    """(z, f, sp, y): z = vcat(xi, xj, e) per edge, f = dense_f's and sp = dense_s's pre-activation, y the layer's output; float64"""
    x, Wf, Ws = np.asarray(x, f64), np.asarray(Wf, f64), np.asarray(Ws, f64)
    parts = [x[t], x[s]] + ([] if e is None else [np.asarray(e, f64)])
    z = np.concatenate(parts, axis=1)
    f = z @ Wf.T + (0.0 if bf is None else np.asarray(bf, f64))
    sp = z @ Ws.T + (0.0 if bs is None else np.asarray(bs, f64))
    y = np.zeros((n, Wf.shape[0]), f64)
    np.add.at(y, t, sigmoid(f) * act(sp, name))
    if residual and x.shape[1] == Wf.shape[0]:
        y = y + x
    return z, f, sp, y


def grad64(s, t, n, x, e, Wf, Ws, bf, bs, name, residual, dy):
    """the composition and its hand-written pullback: dict(y, sp, dx, de, dWf, dWs, dbf, dbs), float64 (de None without e; dbf / dbs are
    computed whether or not the layer has biases)"""
    z, f, sp, y = compose(s, t, n, x, e, Wf, Ws, bf, bs, name, residual)
    dy = np.asarray(dy, f64)
    nin = np.asarray(x).shape[1]
    gf = dy[t] * act(sp, name) * dsigmoid(f)
    gs = dy[t] * sigmoid(f) * dact(sp, name)
    dz = gf @ np.asarray(Wf, f64) + gs @ np.asarray(Ws, f64)
    dx = np.zeros((n, nin), f64)
    np.add.at(dx, t, dz[:, :nin])
    np.add.at(dx, s, dz[:, nin:2 * nin])
    if residual and nin == np.asarray(Wf).shape[0]:
        dx = dx + dy
    return dict(y=y, sp=sp, dx=dx, de=None if e is None else dz[:, 2 * nin:], dWf=gf.T @ z, dWs=gs.T @ z, dbf=gf.sum(axis=0),
                dbs=gs.sum(axis=0))


# ---- the split formulation, in the operands' dtype ------------------------------------------------------------------------------------
def split_fs(x, e, Wf, Ws, bf, bs, dtype):
    """(fs_i, fs_j, fs_e | None), planar [.][2C], from the column blocks of [Wf; Ws]"""
    x, Wf, Ws = np.asarray(x, dtype), np.asarray(Wf, dtype), np.asarray(Ws, dtype)
    nin = x.shape[1]
    blk = lambda a, b: np.concatenate([Wf[:, a:b], Ws[:, a:b]], axis=0)      # noqa: E731
    fs_i = x @ blk(0, nin).T
    if bf is not None:
        fs_i = fs_i + np.concatenate([np.asarray(bf, dtype), np.asarray(bs, dtype)])
    fs_j = x @ blk(nin, 2 * nin).T
    fs_e = None if e is None else np.asarray(e, dtype) @ blk(2 * nin, Wf.shape[1]).T
    c = lambda a: None if a is None else np.ascontiguousarray(a, dtype=dtype)      # noqa: E731
    return c(fs_i), c(fs_j), c(fs_e)


def pre(s, t, fs_i, fs_j, fs_e, C):
    """(f_k, s_k) [E][C] with the forward's additions in the forward's order"""
    f = fs_i[t][:, :C] + fs_j[s][:, :C]
    sp = fs_i[t][:, C:] + fs_j[s][:, C:]
    if fs_e is not None:
        f, sp = f + fs_e[:, :C], sp + fs_e[:, C:]
    return f, sp


def rows(s, t, n, fs_i, fs_j, fs_e, C, name):
    """y [N][C] of gnnmp_propagate_cg_f32 (no residual): the sequential fold of sigmoid(f_k) * act(s_k)"""
    f, sp = pre(s, t, fs_i, fs_j, fs_e, C)
    m = sigmoid(f) * act(sp, name)
    y = np.zeros((n, C), m.dtype)
    for k in range(len(t)):
        y[t[k]] = y[t[k]] + m[k]
    return y


def rows_grad(s, t, n, fs_i, fs_j, fs_e, dy, C, name):
    """(dfs_i, dfs_j, dfs_e | None) of the header's backward, in the dtype of the operands, sums folded sequentially in edge order"""
    f, sp = pre(s, t, fs_i, fs_j, fs_e, C)
    d = dy[t]
    g = np.concatenate([d * act(sp, name) * dsigmoid(f), d * sigmoid(f) * dact(sp, name)], axis=1)
    di, dj = np.zeros((n, 2 * C), g.dtype), np.zeros((n, 2 * C), g.dtype)
    for k in range(len(t)):
        di[t[k]] = di[t[k]] + g[k]
        dj[s[k]] = dj[s[k]] + g[k]
    return di, dj, (None if fs_e is None else g)


def layer(s, t, n, x, e, Wf, Ws, bf, bs, name, residual, dy, dtype=f32):
    """the whole layer and its pullback by the split formulation in `dtype`: dict(y, dx, de, dWf, dWs, dbf, dbs)"""
    x, dy = np.asarray(x, dtype), np.asarray(dy, dtype)
    Wf, Ws = np.asarray(Wf, dtype), np.asarray(Ws, dtype)
    e = None if e is None else np.asarray(e, dtype)
    nin, C = x.shape[1], Wf.shape[0]
    fs_i, fs_j, fs_e = split_fs(x, e, Wf, Ws, bf, bs, dtype)
    y = rows(s, t, n, fs_i, fs_j, fs_e, C, name)
    res = residual and nin == C
    if res:
        y = y + x
    di, dj, de_ = rows_grad(s, t, n, fs_i, fs_j, fs_e, dy, C, name)
    blk = lambda a, b: np.concatenate([Wf[:, a:b], Ws[:, a:b]], axis=0)      # noqa: E731
    dWs_ = [di.T @ x, dj.T @ x] + ([] if e is None else [de_.T @ e])
    dx = di @ blk(0, nin) + dj @ blk(nin, 2 * nin)
    if res:
        dx = dx + dy
    db = di.sum(axis=0)
    return dict(y=y, dx=dx, de=None if e is None else de_ @ blk(2 * nin, Wf.shape[1]),
                dWf=np.concatenate([w[:C] for w in dWs_], axis=1), dWs=np.concatenate([w[C:] for w in dWs_], axis=1), dbf=db[:C], dbs=db[C:])


def rel(got, ref):
    got, ref = np.asarray(got, f64), np.asarray(ref, f64)
    return float(np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-300))


# ---- the graph of the GPU tests ---------------------------------------------------------------------------------------------------------
N_NODES, HUB = 64, 600
NO_IN, NO_OUT, HUB_DST, HUB_SRC = 3, 5, 7, 9


def graph():
    """(s, t) 0-based int64 on 64 nodes, about 1500 edges: >= 12 self loops, >= 28 repeated edges, node 3 without in-edges, node 5 without
    out-edges, destination 7 with 600 in-edges and source 9 with 600 out-edges (beyond the plan's split threshold), shuffled"""
    rng = np.random.default_rng(17)
    n = N_NODES
    srcs, dsts = np.setdiff1d(np.arange(n), [NO_OUT]), np.setdiff1d(np.arange(n), [NO_IN])
    both = np.setdiff1d(np.arange(n), [NO_IN, NO_OUT])
    s, t = rng.choice(srcs, 300), rng.choice(dsts, 300)
    s[:12] = t[:12] = rng.choice(both, 12)                       # self loops
    s[12:40], t[12:40] = s[40:68], t[40:68]                      # repeated edges
    s = np.concatenate([s, rng.choice(srcs, HUB), np.full(HUB, HUB_SRC)])
    t = np.concatenate([t, np.full(HUB, HUB_DST), rng.choice(dsts, HUB)])
    perm = rng.permutation(len(s))
    return s[perm].astype(np.int64), t[perm].astype(np.int64)


def assert_graph(s, t):
    n = N_NODES
    indeg, outdeg = np.bincount(t, minlength=n), np.bincount(s, minlength=n)
    assert len(s) == 1500 and s.dtype == np.int64 and s.min() >= 0 and max(s.max(), t.max()) < n
    assert (s == t).sum() >= 12 and len(s) - len(set(zip(s.tolist(), t.tolist()))) >= 28
    assert indeg[NO_IN] == 0 and outdeg[NO_OUT] == 0
    assert indeg[HUB_DST] >= HUB and outdeg[HUB_SRC] >= HUB


# ---- the kernel-level cases: fs_i, fs_j, fs_e, Δ built on the host ----------------------------------------------------------------------
KERNEL_CS = (1, 3, 6, 8, 64, 260)
# seeds found by find_seed("kernel", ...): the first seed from 0 whose operands meet kernel_condition
KERNEL_SEEDS = {(64, "relu", False): 1, (64, "relu", True): 1, (260, "relu", True): 15}


def kernel_case(C, name, with_e, seed=None):
    """(fs_i, fs_j, fs_e | None, Δ) float32 on graph(): ~ N(0, 1) scaled so that f_k and s_k are O(1)"""
    if seed is None:
        seed = KERNEL_SEEDS.get((C, name, with_e), 0)
    rng = np.random.default_rng([seed, C, ACT_CODE[name], int(with_e)])
    n, E = N_NODES, 1500
    sc = f32(1.0 / np.sqrt(3.0 if with_e else 2.0))
    fs_i = (sc * rng.standard_normal((n, 2 * C))).astype(f32)
    fs_j = (sc * rng.standard_normal((n, 2 * C))).astype(f32)
    fs_e = (sc * rng.standard_normal((E, 2 * C))).astype(f32) if with_e else None
    dy = rng.standard_normal((n, C)).astype(f32)
    return fs_i, fs_j, fs_e, dy


def kernel_ref64(s, t, case, C, name):
    """(dfs_i, dfs_j, dfs_e | None) in float64 on the float32 operands of `case`"""
    fs_i, fs_j, fs_e, dy = [None if a is None else a.astype(f64) for a in case]
    return rows_grad(s, t, N_NODES, fs_i, fs_j, fs_e, dy, C, name)


def kernel_condition(s, t, case, C, name):
    """(worst, kink / dev): worst = the largest norm-wise distance of the float32 restatement of (dfs_i, dfs_j, dfs_e) from float64;
    kink = the smallest |s_k|, dev = the largest float32-float64 deviation of s_k"""
    fs_i, fs_j, fs_e, dy = case
    got = rows_grad(s, t, N_NODES, fs_i, fs_j, fs_e, dy, C, name)
    ref = kernel_ref64(s, t, case, C, name)
    worst = max(rel(g, r) for g, r in zip(got, ref) if g is not None)
    sp32 = pre(s, t, fs_i, fs_j, fs_e, C)[1]
    sp64 = pre(s, t, *[None if a is None else a.astype(f64) for a in (fs_i, fs_j, fs_e)], C)[1]
    dev = float(np.abs(sp32.astype(f64) - sp64).max())
    return worst, float(np.abs(sp64).min()) / max(dev, 2.0 ** -149)


# ---- the layer-level cases -------------------------------------------------------------------------------------------------------------
LAYER_SHAPES = ((5, 0, 5), (6, 3, 6), (4, 1, 7), (64, 16, 64))      # (nin, ein, out)
LAYER_SEEDS = {((64, 16, 64), "relu"): 15}      # find_seed("layer", ...)


def layer_case(shape, name, seed=None):
    """(x, e | None, Wf, Ws, bf, bs, Δ) float32 on graph(): x, e, Δ ~ N(0, 1), weights ~ N(0, 1) / sqrt(2 nin + ein), biases ~ 0.2 N(0, 1)
    (a case without bias drops bf and bs; a case without residual ignores the flag: the operands are the same)"""
    nin, ein, out = shape
    if seed is None:
        seed = LAYER_SEEDS.get((shape, name), 0)
    rng = np.random.default_rng([seed, nin, ein, out, ACT_CODE[name]])
    n, E, K = N_NODES, 1500, 2 * nin + ein
    x = rng.standard_normal((n, nin)).astype(f32)
    e = rng.standard_normal((E, ein)).astype(f32) if ein else None
    Wf, Ws = [(rng.standard_normal((out, K)) / np.sqrt(K)).astype(f32) for _ in range(2)]
    bf, bs = [(0.2 * rng.standard_normal(out)).astype(f32) for _ in range(2)]
    dy = rng.standard_normal((n, out)).astype(f32)
    return x, e, Wf, Ws, bf, bs, dy


WHAT = ("y", "dx", "de", "dWf", "dWs", "dbf", "dbs")


def layer_condition(s, t, case, name, residual, bias):
    """(worst, kink / dev) of one layer case, as kernel_condition, over y, dx, de, dWf, dWs, dbf, dbs"""
    x, e, Wf, Ws, bf, bs, dy = case
    if not bias:
        bf = bs = None
    n = N_NODES
    got = layer(s, t, n, x, e, Wf, Ws, bf, bs, name, residual, dy, f32)
    ref = grad64(s, t, n, x, e, Wf, Ws, bf, bs, name, residual, dy)
    worst = max(rel(got[k], ref[k]) for k in WHAT if got[k] is not None)
    C = Wf.shape[0]
    sp32 = pre(s, t, *split_fs(x, e, Wf, Ws, bf, bs, f32), C)[1]
    dev = float(np.abs(sp32.astype(f64) - ref["sp"]).max())
    return worst, float(np.abs(ref["sp"]).min()) / max(dev, 2.0 ** -149)


def conditioned(cond, name):
    worst, ratio = cond
    return worst <= COND and (name != "relu" or ratio >= MARGIN)


def find_seed(kind, *key):
    """the search the seed tables were filled by: the first seed from 0 on whose operands are well conditioned (layer cases: under every
    combination of residual and bias)"""
    s, t = graph()
    for seed in range(1000):
        if kind == "kernel":
            C, name, with_e = key
            ok = conditioned(kernel_condition(s, t, kernel_case(C, name, with_e, seed), C, name), name)
        else:
            shape, name = key
            case = layer_case(shape, name, seed)
            ok = all(conditioned(layer_condition(s, t, case, name, r, b), name) for r in (False, True) for b in (False, True))
        if ok:
            return seed
    raise AssertionError(f"no well-conditioned seed for {kind} {key}")


# ---- finite differences and the CGCNN step -----------------------------------------------------------------------------------------------
def fd_case(nin, name, seed=1):
    """n = 30, E = 200, ein = 3, C = 5, float64 uniform(-1, 1) operands"""
    rng = np.random.default_rng([seed, nin, ACT_CODE[name]])
    n, E, ein, C = 30, 200, 3, 5
    s, t = rng.integers(0, n, E), rng.integers(0, n, E)
    u = lambda *shape: rng.uniform(-1, 1, shape)      # noqa: E731
    return s, t, n, u(n, nin), u(E, ein), u(C, 2 * nin + ein), u(C, 2 * nin + ein), u(C), u(C), u(n, C)


CGCNN = dict(clouds=4, pts=48, nin=16, ein=8, radius=0.36, seed=5)


def cgcnn_case():
    """(pos [n][3] uniform in the unit cube, graph indicator (0-based), x [n][16], per layer (Wf, Ws, bf, bs), R [clouds][16])"""
    c = CGCNN
    rng = np.random.default_rng(c["seed"])
    n, nin, K = c["clouds"] * c["pts"], c["nin"], 2 * c["nin"] + c["ein"]
    pos = rng.uniform(0, 1, (n, 3)).astype(f32)
    x = rng.standard_normal((n, nin)).astype(f32)
    layers = []
    for _ in range(2):
        Wf, Ws = [(rng.standard_normal((nin, K)) / np.sqrt(K)).astype(f32) for _ in range(2)]
        bf, bs = [(0.2 * rng.standard_normal(nin)).astype(f32) for _ in range(2)]
        layers.append((Wf, Ws, bf, bs))
    R = rng.standard_normal((c["clouds"], nin)).astype(f32)
    return pos, np.repeat(np.arange(c["clouds"]), c["pts"]), x, layers, R


def cgcnn_grad64(s, t, gi, x, e, layers, R, name="softplus"):
    """float64 gradients of loss = Σ mean_pool(h2) .* R through two residual CGConv layers that share the edge features e, on the given
    edge list: (h2, [grad64 dict per layer], dx, de)"""
    n = x.shape[0]
    h1 = compose(s, t, n, x, e, *layers[0], name, True)[3]
    h2 = compose(s, t, n, h1, e, *layers[1], name, True)[3]
    cnt = np.bincount(gi, minlength=R.shape[0])
    dh2 = (np.asarray(R, f64) / cnt[:, None])[gi]
    g2 = grad64(s, t, n, h1, e, *layers[1], name, True, dh2)
    g1 = grad64(s, t, n, x, e, *layers[0], name, True, g2["dx"])
    return h2, [g1, g2], g1["dx"], g1["de"] + g2["de"]
