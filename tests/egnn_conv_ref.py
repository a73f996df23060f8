"""numpy references of tests/test_egnn_conv_ad.py — TEST INFRASTRUCTURE ONLY.

  * forward / backward: EGNNConv (GNNlib/src/layers/conv.jl:459-495) and its hand-derived pullback in the formulation of include/gnnmp.h
    (P, Q, F from the column blocks of ϕe's first weight; z0 = ((P_i + Q_j) + q c) + F; dP, dQ by scatter; the coordinate adjoint with the
    q = 0 convention), in the dtype asked for: float64 is the reference, float32 the restatement whose distance from float64 is the
    CONDITION on the operands of every GPU case.
  * edge_ref / coord_ref / coord_grad_ref / act_grad_z_ref: the four exports one by one.
  * the graph and the operands of every GPU case, the finite-difference case and the small training step.
Edge indices are 0-based here.  Sums over a row are np.add.at: sequential, in edge order, in the operands' dtype."""
import numpy as np

f32, f64 = np.float32, np.float64
ACTS = ("identity", "relu", "softplus", "tanh", "swish")
ACT_CODE = {None: 0, "identity": 0, "relu": 1, "softplus": 2, "tanh": 3, "swish": 4}
MARGIN = 20         # relu's kink is at least this many times farther away than float32 is from float64 (tests/cg_conv_ref.py)
COND = 2e-6         # a fifth of the project's 1e-5 bar
EPS = 1e-6


def sigmoid(v):
    """NNlib.sigmoid: t = exp(-abs(x)); ifelse(x >= 0, inv(1 + t), t / (1 + t)), in v's dtype"""
    one = v.dtype.type(1)
    t = np.exp(-np.abs(v))
    return np.where(v >= 0, one / (one + t), t / (one + t))


def act(v, name):
    if name == "relu":
        return np.where(v < 0, v.dtype.type(0), v)
    if name == "softplus":
        return np.log1p(np.exp(-np.abs(v))) + np.where(v < 0, v.dtype.type(0), v)
    if name == "tanh":
        return np.tanh(v)
    if name == "swish":
        return v * sigmoid(v)
    return v


def dact(v, name):
    """act'(z) from the pre-activation"""
    one = v.dtype.type(1)
    if name == "relu":
        return np.where(v > 0, one, v.dtype.type(0))       # 0 at 0
    if name == "softplus":
        return sigmoid(v)
    if name == "tanh":
        a = np.tanh(v)
        return (one - a) * (one + a)
    if name == "swish":
        sg = sigmoid(v)
        return sg * (one + v * (one - sg))
    return np.ones_like(v)


def rel(got, ref):
    got, ref = np.asarray(got, f64), np.asarray(ref, f64)
    return float(np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-300))


def _c(a, dtype):
    return None if a is None else np.ascontiguousarray(a, dtype=dtype)


def _cast(chain, dtype):
    return [(_c(W, dtype), _c(b, dtype), a) for W, b, a in chain]


def scatter(idx, vals, n):
    out = np.zeros((n,) + vals.shape[1:], vals.dtype)
    np.add.at(out, idx, vals)
    return out


# ---- geometry ------------------------------------------------------------------------------------------------------------------------
def geometry(s, t, x):
    """(d, q, r, den, nk): d_k = x_i − x_j, q_k = Σ_a d² folded from a = 0, r = sqrt(q), den = r + 1e-6, n_k = d / den"""
    d = x[t] - x[s]
    q = np.zeros(len(s), x.dtype)
    for a in range(x.shape[1]):
        q = q + d[:, a] * d[:, a]
    r = np.sqrt(q)
    den = r + x.dtype.type(EPS)
    return d, q, r, den, d / den[:, None]


def edge_ref(s, t, x, P, Q, F, c, name, dtype=f64):
    """(q, z0, a0) of gnnmp_egnn_edge_f32"""
    x, P, Q, F, c = [_c(a, dtype) for a in (x, P, Q, F, c)]
    q = geometry(s, t, x)[1]
    z0 = (P[t] + Q[s]) + q[:, None] * c
    if F is not None:
        z0 = z0 + F
    return q, z0, act(z0, name)


def coord_ref(s, t, n, x, mx, dtype=f64):
    """x' of gnnmp_egnn_coord_f32"""
    x, mx = _c(x, dtype), _c(mx, dtype)
    nk = geometry(s, t, x)[4]
    deg = np.bincount(t, minlength=n)
    agg = scatter(t, mx[:, None] * nk, n)
    return np.where(deg[:, None] > 0, x + agg / np.maximum(deg, 1).astype(dtype)[:, None], x)


def coord_dd(s, t, n, x, dxo, mx, dq):
    """dd_k of the header, with the q = 0 convention"""
    d, q, r, den, _ = geometry(s, t, x)
    deg = np.bincount(t, minlength=n).astype(x.dtype)
    g = (mx / deg[t])[:, None] * dxo[t]
    ok = q > 0
    rs, dens = np.where(ok, r, 1), np.where(ok, den, 1)
    coef = (d * g).sum(axis=1) / (rs * (dens * dens))
    npath = np.where(ok[:, None], g / dens[:, None] - d * coef[:, None], 0)
    return (npath + (2 * dq)[:, None] * d).astype(x.dtype)


def coord_grad_ref(s, t, n, x, dxo, mx, dq, dtype=f64):
    """(dmx, dx) of gnnmp_egnn_coord_grad_f32"""
    x, dxo, mx, dq = [_c(a, dtype) for a in (x, dxo, mx, dq)]
    nk = geometry(s, t, x)[4]
    deg = np.bincount(t, minlength=n).astype(dtype)
    dmx = (nk * dxo[t]).sum(axis=1) / deg[t]
    dd = coord_dd(s, t, n, x, dxo, mx, dq)
    return dmx, (dxo + scatter(t, dd, n)) - scatter(s, dd, n)


def act_grad_z_ref(dy, z, name, dtype=f64):
    return _c(dy, dtype) * dact(_c(z, dtype), name)


# ---- the layer -------------------------------------------------------------------------------------------------------------------------
def _chain(layers, z):
    kept = []
    for W, b, a in layers:
        pre = z @ W.T + (0 if b is None else b)
        kept.append((z, pre))
        z = act(pre, a)
    return z, kept


def _chain_back(layers, kept, dy):
    grads = []
    for (W, b, a), (inp, pre) in zip(reversed(layers), reversed(kept)):
        dz = dy * dact(pre, a)
        grads.append((dz.T @ inp, None if b is None else dz.sum(axis=0)))
        dy = dz @ W
    return grads[::-1], dy


def forward(s, t, n, h, x, e, phi_e, phi_x, phi_h, residual, dtype=f64):
    """everything of the forward, as a dict; h', x' under 'hn', 'xo'"""
    h, x, e = _c(h, dtype), _c(x, dtype), _c(e, dtype)
    pe, px, ph = _cast(phi_e, dtype), _cast(phi_x, dtype), _cast(phi_h, dtype)
    nin = h.shape[1]
    W0, b0, a0n = pe[0]
    A, B, c, D = W0[:, :nin], W0[:, nin:2 * nin], W0[:, 2 * nin], W0[:, 2 * nin + 1:]
    P = h @ A.T + (0 if b0 is None else b0)
    Q = h @ B.T
    F = e @ D.T if e is not None else None
    q, z0, a0 = edge_ref(s, t, x, P, Q, F, c, a0n, dtype)
    mh, kept_e = _chain(pe[1:], a0)
    mx, kept_x = _chain(px, mh)
    h_aggr = scatter(t, mh, n)
    xo = coord_ref(s, t, n, x, mx[:, 0], dtype)
    hn, kept_h = _chain(ph, np.concatenate([h, h_aggr], axis=1))
    if residual:
        hn = h + hn
    return dict(s=s, t=t, n=n, h=h, x=x, e=e, pe=pe, px=px, ph=ph, residual=residual, q=q, z0=z0, a0=a0, mh=mh, mx=mx[:, 0], h_aggr=h_aggr,
                kept_e=kept_e, kept_x=kept_x, kept_h=kept_h, hn=hn, xo=xo, relu_pre=_relu_pre(pe, px, ph, z0, kept_e, kept_x, kept_h))


def _relu_pre(pe, px, ph, z0, kept_e, kept_x, kept_h):
    """the pre-activations that feed a relu, row under row (the layers of one chain have one width)"""
    pres = [z0] + [k[1] for k in kept_e] + [k[1] for k in kept_x] + [k[1] for k in kept_h]
    names = [pe[0][2]] + [l[2] for l in pe[1:]] + [l[2] for l in px] + [l[2] for l in ph]
    pick = [p for p, a in zip(pres, names) if a == "relu"]
    return np.concatenate(pick, axis=0) if pick else np.zeros((0, 1), z0.dtype)


def backward(fw, dhn, dxo):
    """the hand-derived pullback: dict(dh, dx, de, phi_e, phi_x, phi_h), the last three lists of (dW, db | None)"""
    s, t, n, h, x, e = fw["s"], fw["t"], fw["n"], fw["h"], fw["x"], fw["e"]
    dtype = h.dtype
    dhn, dxo = _c(dhn, dtype), _c(dxo, dtype)
    pe, px, ph = fw["pe"], fw["px"], fw["ph"]
    nin = h.shape[1]
    g_h, dcat = _chain_back(ph, fw["kept_h"], dhn)
    dh, dh_aggr = dcat[:, :nin], dcat[:, nin:]
    if fw["residual"]:
        dh = dh + dhn
    dmx, _ = coord_grad_ref(s, t, n, x, dxo, fw["mx"], np.zeros(len(s), dtype), dtype)
    g_x, dmh_x = _chain_back(px, fw["kept_x"], dmx[:, None])
    dmh = dh_aggr[t] + dmh_x
    g_e, da0 = _chain_back(pe[1:], fw["kept_e"], dmh)
    W0, b0, a0n = pe[0]
    dz0 = da0 * dact(fw["z0"], a0n)
    dP, dQ = scatter(t, dz0, n), scatter(s, dz0, n)
    blocks = [dP.T @ h, dQ.T @ h, dz0.T @ fw["q"][:, None]] + ([] if e is None else [dz0.T @ e])
    g_e = [(np.concatenate(blocks, axis=1), None if b0 is None else dP.sum(axis=0))] + g_e
    dh = dh + (dP @ W0[:, :nin] + dQ @ W0[:, nin:2 * nin])
    dq = dz0 @ W0[:, 2 * nin]
    de = None if e is None else dz0 @ W0[:, 2 * nin + 1:]
    _, dx = coord_grad_ref(s, t, n, x, dxo, fw["mx"], dq, dtype)
    return dict(dh=dh, dx=dx, de=de, phi_e=g_e, phi_x=g_x, phi_h=g_h)


def flat(fw, bw):
    """{name: array} of everything a layer test compares"""
    out = dict(hn=fw["hn"], xo=fw["xo"], dh=bw["dh"], dx=bw["dx"])
    if bw["de"] is not None:
        out["de"] = bw["de"]
    for name in ("phi_e", "phi_x", "phi_h"):
        for k, (dW, db) in enumerate(bw[name]):
            out[f"dW {name}[{k}]"] = dW
            if db is not None:
                out[f"db {name}[{k}]"] = db
    return out


def layer64(s, t, n, case, residual):
    h, x, e, pe, px, ph, dhn, dxo = case
    fw = forward(s, t, n, h, x, e, pe, px, ph, residual, f64)
    return fw, flat(fw, backward(fw, dhn, dxo))


def condition(got, ref, relu32=None, relu64=None):
    """(worst, kink / dev) as tests/cg_conv_ref.py: worst = the largest norm-wise distance of a float32 restatement from float64 over the
    compared quantities; kink / dev = the smallest, over the rows that feed a relu, of (the row's smallest |pre-activation|) / (the row's
    largest float32-float64 deviation) — row by row, because the rows differ in scale: a hub's row sums 600 messages and deviates by
    1e-4 where an ordinary row deviates by 1e-7"""
    worst = max(rel(got[k], ref[k]) for k in ref)
    if relu64 is None or relu64.size == 0:
        return worst, float("inf")
    dev = np.abs(relu32.astype(f64) - relu64).max(axis=1)
    return worst, float((np.abs(relu64).min(axis=1) / np.maximum(dev, 2.0 ** -149)).min())


def layer_condition(s, t, n, case, residual):
    h, x, e, pe, px, ph, dhn, dxo = case
    fw32 = forward(s, t, n, h, x, e, pe, px, ph, residual, f32)
    got = flat(fw32, backward(fw32, dhn, dxo))
    fw64, ref = layer64(s, t, n, case, residual)
    return condition(got, ref, fw32["relu_pre"], fw64["relu_pre"])


def conditioned(cond):
    return cond[0] <= COND and cond[1] >= MARGIN


# ---- the graph of the GPU tests ---------------------------------------------------------------------------------------------------------
N_NODES, HUB = 700, 600
NO_IN, NO_OUT, HUB_DST, HUB_SRC, SELF, COIN_A, COIN_B = 3, 5, 7, 9, 11, 20, 431
SPACING, JITTER = 0.5, 0.2      # lattice pitch; jitter as a share of it: distinct lattice points stay >= (1 − 2 JITTER) SPACING = 0.3 apart


def graph():
    """(s, t) 0-based int64 on 700 nodes, 2603 edges: one self loop (node 11), >= 20 repeated edges, the distinct nodes 20 and 431 — at
    identical coordinates — connected both ways, node 3 without in-edges, node 5 without out-edges, destination 7 with 600 in-edges and
    source 9 with 600 out-edges (beyond the plan's split threshold), shuffled.  No other edge joins a node to itself."""
    rng = np.random.default_rng(23)
    n = N_NODES
    srcs, dsts = np.setdiff1d(np.arange(n), [NO_OUT]), np.setdiff1d(np.arange(n), [NO_IN])
    s, t = rng.choice(srcs, 1400), rng.choice(dsts, 1400)
    s[:20], t[:20] = s[20:40], t[20:40]                           # repeated edges
    s = np.concatenate([s, rng.choice(np.setdiff1d(srcs, [HUB_DST]), HUB), np.full(HUB, HUB_SRC), [SELF, COIN_A, COIN_B]])
    t = np.concatenate([t, np.full(HUB, HUB_DST), rng.choice(np.setdiff1d(dsts, [HUB_SRC]), HUB), [SELF, COIN_B, COIN_A]])
    loops = np.flatnonzero((s == t) & (np.arange(len(s)) != len(s) - 3))
    for k in loops:                                               # an accidental self loop: move its source on
        while s[k] == t[k] or s[k] == NO_OUT:
            s[k] = (s[k] + 1) % n
    coin = ((s == COIN_A) & (t == COIN_B)) | ((s == COIN_B) & (t == COIN_A))
    coin[-2:] = False
    keep = ~coin                                                  # the coincident pair is joined by its own two edges only
    s, t = s[keep], t[keep]
    perm = rng.permutation(len(s))
    return s[perm].astype(np.int64), t[perm].astype(np.int64)


def assert_graph(s, t):
    n = N_NODES
    indeg, outdeg = np.bincount(t, minlength=n), np.bincount(s, minlength=n)
    assert s.dtype == np.int64 and s.min() >= 0 and max(s.max(), t.max()) < n and len(s) > 2600
    assert (s == t).sum() == 1 and s[s == t][0] == SELF
    assert len(s) - len(set(zip(s.tolist(), t.tolist()))) >= 20
    assert indeg[NO_IN] == 0 and outdeg[NO_OUT] == 0
    assert indeg[HUB_DST] >= HUB and outdeg[HUB_SRC] >= HUB
    assert ((s == COIN_A) & (t == COIN_B)).sum() == 1 and ((s == COIN_B) & (t == COIN_A)).sum() == 1


def coords(Dx, n=N_NODES, seed=0, coincident=True):
    """[n][Dx] float32 on a jittered lattice of pitch SPACING (the smallest cube of side^Dx >= n points): every pair of distinct lattice
    points is at least 0.3 apart.  Node COIN_B sits exactly on node COIN_A."""
    side = 1
    while side ** Dx < n:
        side += 1
    rng = np.random.default_rng([seed, Dx, n])
    idx = np.arange(n)
    cell = np.stack([(idx // side ** a) % side for a in range(Dx)], axis=1)
    x = (SPACING * (cell + rng.uniform(-JITTER, JITTER, (n, Dx)))).astype(f32)
    if coincident:
        x[COIN_B] = x[COIN_A]
    return x


def q_zero(s, t):
    """the edges with q = 0 on coords(): the self loop and the coincident pair"""
    return (s == t) | ((s == COIN_A) & (t == COIN_B)) | ((s == COIN_B) & (t == COIN_A))


# ---- the kernel-level cases -------------------------------------------------------------------------------------------------------------
HIDS = (1, 3, 6, 8, 64, 260)
DXS = (1, 2, 3, 4, 7, 16)
C_SCALE = 0.05      # q reaches ~60 on the lattice: c is scaled so that q c stays O(1)


def edge_case(hid, name, with_f, seed=0):
    """(x [N][3], P, Q [N][hid], F [E][hid] | None, c [hid]) float32 on graph(): z0 is O(1)"""
    rng = np.random.default_rng([seed, hid, ACT_CODE[name], int(with_f)])
    n, E = N_NODES, len(graph()[0])
    sc = f32(1.0 / np.sqrt(4.0 if with_f else 3.0))
    P, Q = [(sc * rng.standard_normal((n, hid))).astype(f32) for _ in range(2)]
    F = (sc * rng.standard_normal((E, hid))).astype(f32) if with_f else None
    c = (C_SCALE * sc * rng.standard_normal(hid)).astype(f32)
    return coords(3), P, Q, F, c


def coord_case(Dx, seed=0):
    """(x [N][Dx], Δx' [N][Dx], mx [E], dq [E]) float32 on graph()"""
    rng = np.random.default_rng([seed, Dx])
    n, E = N_NODES, len(graph()[0])
    return coords(Dx), rng.standard_normal((n, Dx)).astype(f32), rng.standard_normal(E).astype(f32), (0.1 * rng.standard_normal(E)).astype(f32)


ACT_NS = (1, 5, 4099)


def act_case(n, name, seed=0):
    """(dy, z) float32 [n]; relu: z exactly as given, no kink to keep away from (the export reads z, it does not compute it)"""
    rng = np.random.default_rng([seed, n, ACT_CODE[name]])
    return rng.standard_normal(n).astype(f32), (2.0 * rng.standard_normal(n)).astype(f32)


# ---- the layer-level cases --------------------------------------------------------------------------------------------------------------
# (nin, ein, out, hid) and the activations of (ϕe, ϕx, ϕh); None = identity.  The first and the last are the layer's defaults (swish);
# the middle one puts tanh, identity, softplus and relu where the default has swish.  relu sits on N rows (ϕh): among the 2600 x 12
# pre-activations of an E-row layer the smallest lies closer to 0 than float32 is to float64, whatever the seed — no layer case could
# meet MARGIN there; relu on E rows is covered at kernel level (K1, gnnmp_act_grad_z_f32), where z is an input
LAYER_SHAPES = ((4, 0, 4, 8), (6, 3, 5, 12), (64, 16, 64, 64))
LAYER_ACTS = {
    (4, 0, 4, 8): (("swish", "swish"), ("swish", None), ("swish", None)),
    (6, 3, 5, 12): (("tanh", None), ("softplus", None), ("relu", "tanh")),
    (64, 16, 64, 64): (("swish", "swish"), ("swish", None), ("swish", None)),
}
LAYER_CASES = [(shape, residual) for shape in LAYER_SHAPES for residual in ((False, True) if shape[0] == shape[2] else (False,))]
LAYER_SEEDS = {(64, 16, 64, 64): 1}      # find_seed(shape): the first seed from 0 whose operands meet layer_condition; 0 unless listed


def make_chains(rng, nin, ein, out, hid, acts, dtype=f32, c_scale=C_SCALE):
    """(ϕe, ϕx, ϕh) with EGNNConv's shapes: weights ~ N(0, 1) / sqrt(fan in), biases ~ 0.2 N(0, 1), the last ϕx layer hid -> 1 without
    bias; the q column of ϕe's first weight scaled by c_scale"""
    def mk(o, i, a, bias=True):
        W = (rng.standard_normal((o, i)) / np.sqrt(i)).astype(dtype)
        return [W, (0.2 * rng.standard_normal(o)).astype(dtype) if bias else None, a]
    ae, ax, ah = acts
    pe = [mk(hid, 2 * nin + 1 + ein, ae[0]), mk(hid, hid, ae[1])]
    pe[0][0][:, 2 * nin] *= dtype(c_scale)
    px = [mk(hid, hid, ax[0]), mk(1, hid, ax[1], bias=False)]
    ph = [mk(hid, nin + hid, ah[0]), mk(out, hid, ah[1])]
    return [tuple(l) for l in pe], [tuple(l) for l in px], [tuple(l) for l in ph]


def layer_case(shape, seed=None):
    """(h, x [N][3], e | None, ϕe, ϕx, ϕh, Δh', Δx') float32 on graph()"""
    nin, ein, out, hid = shape
    if seed is None:
        seed = LAYER_SEEDS.get(shape, 0)
    rng = np.random.default_rng([seed, nin, ein, out, hid])
    n, E = N_NODES, len(graph()[0])
    h = rng.standard_normal((n, nin)).astype(f32)
    e = rng.standard_normal((E, ein)).astype(f32) if ein else None
    pe, px, ph = make_chains(rng, nin, ein, out, hid, LAYER_ACTS[shape])
    return h, coords(3), e, pe, px, ph, rng.standard_normal((n, out)).astype(f32), rng.standard_normal((n, 3)).astype(f32)


def find_seed(shape):
    s, t = graph()
    for seed in range(200):
        case = layer_case(shape, seed)
        if all(conditioned(layer_condition(s, t, N_NODES, case, r)) for r in ((False, True) if shape[0] == shape[2] else (False,))):
            return seed
    raise AssertionError(f"no well-conditioned seed for {shape}")


# ---- finite differences -------------------------------------------------------------------------------------------------------------------
def fd_case(name, seed=1):
    """n = 12, E = 40, nin = 4, ein = 2, out = 4, hid = 5, Dx = 3, float64; `name` is the activation of both ϕe layers, the rest is swish.
    No self loop and no coincident points: q > 0 on every edge (the q = 0 convention is not a derivative)"""
    rng = np.random.default_rng([seed, ACT_CODE[name]])
    n, E, nin, ein, out, hid = 12, 40, 4, 2, 4, 5
    s = rng.integers(0, n, E)
    t = (s + rng.integers(1, n, E)) % n
    u = lambda *shape: rng.uniform(-1, 1, shape)      # noqa: E731
    x = coords(3, n=n, seed=seed, coincident=False).astype(f64) * 2.0
    pe, px, ph = make_chains(rng, nin, ein, out, hid, ((name, name), ("swish", None), ("swish", None)), dtype=f64, c_scale=0.3)
    return s, t, n, u(n, nin), x, u(E, ein), pe, px, ph, u(n, out), u(n, 3)


# ---- the small training step ----------------------------------------------------------------------------------------------------------------
STEP = dict(clouds=4, pts=48, nin=16, radius=0.33, seed=5)


def step_case():
    """(pos [192][3], graph indicator (0-based), h [192][16], [(ϕe, ϕx, ϕh)] * 2, R [clouds][16], Rx [192][3]): each cloud is a jittered
    4 x 4 x 3 lattice of pitch 0.25 in the unit cube — neighbours are at least 0.15 apart"""
    c = STEP
    rng = np.random.default_rng(c["seed"])
    n, nin = c["clouds"] * c["pts"], c["nin"]
    idx = np.arange(c["pts"])
    cell = np.stack([idx % 4, (idx // 4) % 4, idx // 16], axis=1)
    pos = np.concatenate([0.25 * (cell + rng.uniform(-JITTER, JITTER, (c["pts"], 3))) for _ in range(c["clouds"])]).astype(f32)
    h = rng.standard_normal((n, nin)).astype(f32)
    layers = [make_chains(rng, nin, 0, nin, 2 * nin, (("swish", "swish"), ("swish", None), ("swish", None)), c_scale=1.0) for _ in range(2)]
    return pos, np.repeat(np.arange(c["clouds"]), c["pts"]), h, layers, rng.standard_normal((c["clouds"], nin)).astype(f32), \
        rng.standard_normal((n, 3)).astype(f32)


def step_grad64(s, t, gi, h, pos, layers, R, Rx):
    """float64 gradients of loss = Σ mean_pool(h2) .* R + Σ x2 .* Rx through two residual EGNNConv layers on the given edge list:
    (h2, x2, [backward dict per layer], dh, dpos)"""
    n = h.shape[0]
    fw1 = forward(s, t, n, h, pos, None, *layers[0], True, f64)
    fw2 = forward(s, t, n, fw1["hn"], fw1["xo"], None, *layers[1], True, f64)
    cnt = np.bincount(gi, minlength=R.shape[0])
    dh2 = (np.asarray(R, f64) / cnt[:, None])[gi]
    b2 = backward(fw2, dh2, np.asarray(Rx, f64))
    b1 = backward(fw1, b2["dh"], b2["dx"])
    return fw2["hn"], fw2["xo"], [b1, b2], b1["dh"], b1["dx"]
