"""numpy references of tests/test_nn_conv_ad.py — TEST INFRASTRUCTURE ONLY.

  * compose / grad64: NNConv as the reference composes it (GNNlib/src/layers/conv.jl:260-273: we = nn(e), W_k = reshape(we_k, out, in),
    m = aggr_k W_k x_j, σ.(weight * x .+ m .+ bias)) restated in float64, and its pullback written by hand.
  * rows_grad64 / rows_grad32: the two formulas of include/gnnmp.h for gnnmp_nn_conv_grad_f32 — dwe[k][o + Dout c] = Δ[i][o] x[j][c],
    dx[j][c] = Σ_k Σ_o we[k][o + Dout c] Δ[i][o] — in float64, and in float32 IN THE HEADER'S SUMMATION ORDER (per-lane sequential folds,
    then a butterfly across the lanes of the group).
  * layer32: the whole layer and its pullback in float32, every fold in the order the kernels use.
  * the operands of every GPU case, with seeds picked by a search on the CPU (find_seed) for inputs on which float32 stays within COND of
    float64 and every relu pre-activation stays away from the kink.
The graph is the multigraph of tests/cg_conv_ref.py.  Edge indices are 0-based here; `nn` is a list of (W, b, act) with act None or "relu"."""
import numpy as np

from cg_conv_ref import COND, MARGIN, N_NODES, assert_graph, graph, rel  # noqa: F401

f32, f64 = np.float32, np.float64
N_EDGES = 1500


def relu(v):
    return np.where(v < 0, v.dtype.type(0), v)


def drelu(v):
    return np.where(v > 0, v.dtype.type(1), v.dtype.type(0))      # 0 at 0, as gnnmp_act_grad_f32


def inv_count(t, n, dtype):
    return (1.0 / np.maximum(np.bincount(t, minlength=n), 1)).astype(dtype)


# ---- the reference's composition, float64 -----------------------------------------------------------------------------------------
def nn_forward(e, nn, dtype):
    """(we, [(input, pre-activation) per layer]) of the Dense chain in `dtype`"""
    h, trace = np.asarray(e, dtype), []
    for W, b, act in nn:
        pre = h @ np.asarray(W, dtype).T + np.asarray(b, dtype)
        trace.append((h, pre))
        h = relu(pre) if act == "relu" else pre
    return h, trace


def compose(s, t, n, x, e, nn, W, b, sigma, aggr):
    """(we, trace, m, z, y) in float64: z the layer's pre-activation"""
    x, W = np.asarray(x, f64), np.asarray(W, f64)
    out, nin = W.shape
    we, trace = nn_forward(e, nn, f64)
    Wk = we.reshape(len(s), nin, out)                       # element (o, c) at o + out * c: [k][c][o]
    msg = np.einsum("kco,kc->ko", Wk, x[s])
    m = np.zeros((n, out), f64)
    np.add.at(m, t, msg)
    if aggr == "mean":
        m = m * inv_count(t, n, f64)[:, None]
    z = x @ W.T + m + (0.0 if b is None else np.asarray(b, f64))
    return we, trace, m, z, (relu(z) if sigma == "relu" else z)


def nn_backward(d, nn, trace, dtype):
    """(de, [(dW, db) per layer]) of the Dense chain from the cotangent of its output"""
    grads = []
    for (W, b, act), (inp, pre) in zip(reversed(nn), reversed(trace)):
        if act == "relu":
            d = d * drelu(pre)
        grads.append((d.T @ inp, d.sum(axis=0)))
        d = d @ np.asarray(W, dtype)
    return d, grads[::-1]


def grad64(s, t, n, x, e, nn, W, b, sigma, aggr, dy):
    """the composition and its hand-written pullback, float64: dict(y, z, pres, dx, de, dW, db, nn = [(dWn, dbn), ...]) (db is computed
    whether or not the layer has a bias; pres: the pre-activations of nn's relu layers)"""
    we, trace, m, z, y = compose(s, t, n, x, e, nn, W, b, sigma, aggr)
    x, W, dy = np.asarray(x, f64), np.asarray(W, f64), np.asarray(dy, f64)
    out, nin = W.shape
    dz = dy * drelu(z) if sigma == "relu" else dy
    dm = dz * inv_count(t, n, f64)[:, None] if aggr == "mean" else dz
    dx_m, dwe = rows_grad64(s, t, n, x, we, dm, nin, out)
    de, nng = nn_backward(dwe, nn, trace, f64)
    pres = [pre for (_, _, act), (_, pre) in zip(nn, trace) if act == "relu"]
    return dict(y=y, z=z, pres=pres, dx=dz @ W + dx_m, de=de, dW=dz.T @ x, db=dz.sum(axis=0), nn=nng)


# ---- the export's two formulas ---------------------------------------------------------------------------------------------------------
def rows_grad64(s, t, n, x, we, dm, Din, Dout):
    """(dx [n][Din], dwe [E][Dout * Din]) in float64"""
    x, we, dm = np.asarray(x, f64), np.asarray(we, f64), np.asarray(dm, f64)
    E = len(s)
    dwe = (x[s][:, :, None] * dm[t][:, None, :]).reshape(E, Din * Dout)      # [k][c][o]
    per_edge = np.einsum("kco,ko->kc", we.reshape(E, Din, Dout), dm[t])
    dx = np.zeros((n, Din), f64)
    np.add.at(dx, s, per_edge)
    return dx, dwe


def lane_geometry(Dout):
    """(VEC, G, U) of csrc/nn_grad.hip for 16-byte aligned arrays"""
    vec = 4 if Dout % 4 == 0 else (2 if Dout % 2 == 0 else 1)
    lanes, G = Dout // vec, 1
    while G < lanes and G < 64:
        G *= 2
    return vec, G, (2 if vec == 4 else 4)


def rows_grad32(s, t, n, x, we, dm, Din, Dout):
    """(dx, dwe) in float32 in the header's summation order: lane l owns o = (tt G + l) VEC + q; each lane folds its products
    sequentially — edges of source j in original order in batches of U; within a batch tt ascending, then the batch's edges, then q —
    and the G lane partials are summed by a butterfly (m = G/2 ... 1).  Every in-channel c is folded alike: vectorised over c and lanes."""
    x, we, dm = np.asarray(x, f32), np.asarray(we, f32), np.asarray(dm, f32)
    E = len(s)
    VEC, G, U = lane_geometry(Dout)
    dwe = (x[s][:, :, None] * dm[t][:, None, :]).reshape(E, Din * Dout)      # one product each: no order
    Wk = we.reshape(E, Din, Dout)
    T = -(-Dout // (G * VEC))
    lanes = np.arange(G)
    dx = np.zeros((n, Din), f32)
    order = np.argsort(s, kind="stable")
    bounds = np.searchsorted(s[order], np.arange(n + 1))
    for j in range(n):
        ks = order[bounds[j]:bounds[j + 1]]
        p = np.zeros((G, Din), f32)
        for b0 in range(0, len(ks), U):
            for tt in range(T):
                for k in ks[b0:b0 + U]:
                    for q in range(VEC):
                        o = (tt * G + lanes) * VEC + q
                        ok = o < Dout
                        oc = np.where(ok, o, 0)
                        prod = Wk[k][:, oc].T * dm[t[k]][oc][:, None]      # [G][Din], rounded
                        p = np.where(ok[:, None], p + prod, p)
        m = G // 2
        while m >= 1:
            p = p + p[lanes ^ m]
            m //= 2
        dx[j] = p[0]
    return dx, dwe


# ---- the kernel-level cases ------------------------------------------------------------------------------------------------------------------
# a single lane; tails in both dimensions; Din = 33: five in-channel tiles of 8, the last with one channel; Dout = 70:
# 35 8-byte lanes; the workload's own 64 x 64 — and two at which a lane owns more than one vector of outputs (65 lanes' worth)
KERNEL_SHAPES = ((1, 1), (3, 5), (8, 8), (16, 4), (5, 16), (33, 20), (20, 70), (64, 64), (3, 130), (2, 260))
KERNEL_SEEDS = {}      # find_seed("kernel", ...): seed 0 meets the condition at every shape


def kernel_case(Din, Dout, seed=None):
    """(x, we, Δ) float32 on graph(): x, Δ ~ N(0, 1), we ~ N(0, 1 / Din)"""
    if seed is None:
        seed = KERNEL_SEEDS.get((Din, Dout), 0)
    rng = np.random.default_rng([seed, Din, Dout])
    x = rng.standard_normal((N_NODES, Din)).astype(f32)
    we = (rng.standard_normal((N_EDGES, Dout * Din)) / np.sqrt(Din)).astype(f32)
    dm = rng.standard_normal((N_NODES, Dout)).astype(f32)
    return x, we, dm


def kernel_ref64(s, t, case, Din, Dout):
    return rows_grad64(s, t, N_NODES, *case, Din, Dout)


def kernel_condition(s, t, case, Din, Dout):
    """the largest norm-wise distance of the float32 restatement of (dx, dwe) from float64"""
    got = rows_grad32(s, t, N_NODES, *case, Din, Dout)
    return max(rel(g, r) for g, r in zip(got, kernel_ref64(s, t, case, Din, Dout)))


# ---- the layer-level cases ---------------------------------------------------------------------------------------------------------------------
LAYER_SHAPES = ((5, 2, 5), (4, 1, 7), (16, 8, 16))      # (in, ein, out)
HIDDEN = 6                                                # width of the first of two Dense layers
LAYER_SEEDS = {((16, 8, 16), 2): 1}                       # find_seed("layer", shape, depth): seed 0 elsewhere
WHAT = ("y", "dx", "de", "dW", "db")


def layer_case(shape, depth, seed=None):
    """(x, e, nn, W, b, Δ) float32 on graph(): x, e, Δ ~ N(0, 1); every weight ~ N(0, 1) / sqrt(fan-in), nn's last layer scaled by a
    further 1 / sqrt(in) (so that W_k x_j is O(1)); biases ~ 0.2 N(0, 1).  depth 1: nn = [Dense(ein => out in)]; depth 2:
    [Dense(ein => 6, relu), Dense(6 => out in)]"""
    nin, ein, out = shape
    if seed is None:
        seed = LAYER_SEEDS.get((shape, depth), 0)
    rng = np.random.default_rng([seed, nin, ein, out, depth])
    x = rng.standard_normal((N_NODES, nin)).astype(f32)
    e = rng.standard_normal((N_EDGES, ein)).astype(f32)
    widths = [ein] + ([HIDDEN] if depth == 2 else []) + [out * nin]
    nn = []
    for i, (a, c) in enumerate(zip(widths[:-1], widths[1:])):
        last = i == len(widths) - 2
        Wn = (rng.standard_normal((c, a)) / np.sqrt(a * (nin if last else 1))).astype(f32)
        bn = (0.2 * rng.standard_normal(c) / np.sqrt(nin if last else 1)).astype(f32)
        nn.append((Wn, bn, None if last else "relu"))
    W = (rng.standard_normal((out, nin)) / np.sqrt(nin)).astype(f32)
    b = (0.2 * rng.standard_normal(out)).astype(f32)
    dy = rng.standard_normal((N_NODES, out)).astype(f32)
    return x, e, nn, W, b, dy


def layer32(s, t, n, x, e, nn, W, b, sigma, aggr, dy):
    """the whole layer and its pullback in float32: the forward's sums fold in edge order (nn_rows_kernel: a message's products in
    channel order, messages in edge order), the export's in the header's order (rows_grad32), the dense products as numpy forms them"""
    x, W, dy = np.asarray(x, f32), np.asarray(W, f32), np.asarray(dy, f32)
    out, nin = W.shape
    we, trace = nn_forward(e, nn, f32)
    Wk = we.reshape(len(s), nin, out)
    msg = np.zeros((len(s), out), f32)
    for c in range(nin):
        msg = msg + Wk[:, c, :] * x[s][:, c:c + 1]
    m = np.zeros((n, out), f32)
    for k in range(len(s)):
        m[t[k]] = m[t[k]] + msg[k]
    if aggr == "mean":
        m = m * inv_count(t, n, f32)[:, None]
    z = x @ W.T + m
    if b is not None:
        z = z + np.asarray(b, f32)
    y = relu(z) if sigma == "relu" else z
    dz = dy * drelu(z) if sigma == "relu" else dy
    dm = dz * inv_count(t, n, f32)[:, None] if aggr == "mean" else dz
    dx_m, dwe = rows_grad32(s, t, n, x, we, dm, nin, out)
    de, nng = nn_backward(dwe, nn, trace, f32)
    pres = [pre for (_, _, act), (_, pre) in zip(nn, trace) if act == "relu"]
    return dict(y=y, z=z, pres=pres, dx=dz @ W + dx_m, de=de, dW=dz.T @ x, db=dz.sum(axis=0), nn=nng)


def flat(res, bias=True):
    """[(name, array)] of everything a layer case compares"""
    items = [(k, res[k]) for k in WHAT if bias or k != "db"]
    for i, (dWn, dbn) in enumerate(res["nn"]):
        items += [(f"nn{i}.dW", dWn), (f"nn{i}.db", dbn)]
    return items


def layer_condition(s, t, case, sigma, aggr, bias):
    """(worst, kink / dev): worst = the largest norm-wise distance of the float32 restatement from float64 over y, dx, de, dW, db and nn's
    gradients; kink = the smallest |pre-activation| of any relu (nn's hidden layer, and the layer's own z under σ = relu), dev = the
    largest float32-float64 deviation of those pre-activations (inf when there is no relu)"""
    x, e, nn, W, b, dy = case
    if not bias:
        b = None
    got = layer32(s, t, N_NODES, x, e, nn, W, b, sigma, aggr, dy)
    ref = grad64(s, t, N_NODES, x, e, nn, W, b, sigma, aggr, dy)
    worst = max(rel(g, r) for (_, g), (_, r) in zip(flat(got, bias), flat(ref, bias)))
    pairs = list(zip(got["pres"], ref["pres"])) + ([(got["z"], ref["z"])] if sigma == "relu" else [])
    ratio = np.inf
    for p32, p64 in pairs:
        dev = float(np.abs(p32.astype(f64) - p64).max())
        ratio = min(ratio, float(np.abs(p64).min()) / max(dev, 2.0 ** -149))
    return worst, ratio


def conditioned(cond):
    worst, ratio = cond
    return worst <= COND and ratio >= MARGIN


LAYER_VARIANTS = [(sigma, aggr, bias) for sigma in (None, "relu") for aggr in ("+", "mean") for bias in (True, False)]


def find_seed(kind, *key):
    """the search the seed tables were filled by: the first seed from 0 on whose operands are well conditioned (layer cases: under every
    combination of σ, aggr and bias)"""
    s, t = graph()
    for seed in range(1000):
        if kind == "kernel":
            ok = kernel_condition(s, t, kernel_case(*key, seed), *key) <= COND
        else:
            case = layer_case(*key, seed)
            ok = all(conditioned(layer_condition(s, t, case, *v)) for v in LAYER_VARIANTS)
        if ok:
            return seed
    raise AssertionError(f"no well-conditioned seed for {kind} {key}")


# ---- finite differences ---------------------------------------------------------------------------------------------------------------------
FD_SEEDS = {}      # (depth, sigma): seed 1 keeps every relu pre-activation at least 100 h from the kink, under + and under mean


def fd_case(depth, sigma, seed=None):
    """n = 30, E = 200, ein = 3, in = 4, out = 5, float64 uniform(-1, 1) operands (nn's weights scaled by 1 / 2)"""
    if seed is None:
        seed = FD_SEEDS.get((depth, sigma), 1)
    rng = np.random.default_rng([seed, depth])
    n, E, ein, nin, out = 30, 200, 3, 4, 5
    s, t = rng.integers(0, n, E), rng.integers(0, n, E)
    u = lambda *shape: rng.uniform(-1, 1, shape)      # noqa: E731
    widths = [ein] + ([HIDDEN] if depth == 2 else []) + [out * nin]
    nn = [(0.5 * u(c, a), 0.5 * u(c), None if i == len(widths) - 2 else "relu") for i, (a, c) in enumerate(zip(widths[:-1], widths[1:]))]
    return s, t, n, u(n, nin), u(E, ein), nn, u(out, nin), u(out), u(n, out)


# ---- a small MPNN step ------------------------------------------------------------------------------------------------------------------------
MPNN = dict(clouds=4, pts=48, nin=8, ein=4, hidden=16, radius=0.3, seed=3)


def mpnn_case():
    """(pos [n][3] uniform in the unit cube, graph indicator (0-based), x [n][8], per layer (nn, W, b), R [clouds][8])"""
    c = MPNN
    rng = np.random.default_rng(c["seed"])
    n, nin = c["clouds"] * c["pts"], c["nin"]
    pos = rng.uniform(0, 1, (n, 3)).astype(f32)
    x = rng.standard_normal((n, nin)).astype(f32)
    layers = []
    for _ in range(2):
        W1 = (rng.standard_normal((c["hidden"], c["ein"])) / np.sqrt(c["ein"])).astype(f32)
        b1 = (0.2 * rng.standard_normal(c["hidden"])).astype(f32)
        W2 = (rng.standard_normal((nin * nin, c["hidden"])) / np.sqrt(c["hidden"] * nin)).astype(f32)
        b2 = (0.2 * rng.standard_normal(nin * nin) / np.sqrt(nin)).astype(f32)
        W = (rng.standard_normal((nin, nin)) / np.sqrt(nin)).astype(f32)
        b = (0.2 * rng.standard_normal(nin)).astype(f32)
        layers.append(([(W1, b1, "relu"), (W2, b2, None)], W, b))
    R = rng.standard_normal((c["clouds"], nin)).astype(f32)
    return pos, np.repeat(np.arange(c["clouds"]), c["pts"]), x, layers, R


def mpnn_grad64(s, t, gi, x, e, layers, R):
    """float64 gradients of loss = Σ mean_pool(h2) .* R through two NNConv(8 => 8, nn, relu; aggr = mean) layers that share the edge
    features e, on the given edge list: (h2, [grad64 dict per layer], dx, de, smallest |relu pre-activation|)"""
    n = x.shape[0]
    h1 = compose(s, t, n, x, e, *layers[0], "relu", "mean")[4]
    h2 = compose(s, t, n, h1, e, *layers[1], "relu", "mean")[4]
    cnt = np.bincount(gi, minlength=R.shape[0])
    dh2 = (np.asarray(R, f64) / cnt[:, None])[gi]
    g2 = grad64(s, t, n, h1, e, *layers[1], "relu", "mean", dh2)
    g1 = grad64(s, t, n, x, e, *layers[0], "relu", "mean", g2["dx"])
    kink = min(float(np.abs(p).min()) for g in (g1, g2) for p in g["pres"] + [g["z"]])
    return h2, [g1, g2], g1["dx"], g1["de"] + g2["de"], kink
