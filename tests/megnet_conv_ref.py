"""A float64 numpy model of MEGNetConv's training path (tests/test_megnet_conv_ad.py): the layer with both outputs (megnet_conv,
GNNlib/src/layers/conv.jl:356-368), the formulas of the three exports of csrc/megnet.hip as include/gnnmp.h states them, and their
gradients derived by hand.  Every function takes a dtype, so the same text is the float32 restatement the input conditions use.
Edge k: s[k] -> t[k], 0-based.  The max / min pullback uses the reference's rule: Δ where m_k == y_i, every tying copy included."""
import numpy as np

f32, f64 = np.float32, np.float64
ACTS = ("identity", "relu", "softplus", "tanh", "swish")
ACT_CODE = {"identity": 0, "relu": 1, "softplus": 2, "tanh": 3, "swish": 4}
AGGRS = ("+", "mean", "max", "min")
AGGR_CODE = {"+": 0, "mean": 1, "max": 2, "min": 3}
COND = 2e-6         # a fifth of the project's 1e-5 bar
KINK = 1e-3         # relu: every pre-activation at least this far from 0; max / min: the winner beats the runner-up by at least this
U32 = 2.0 ** -24    # float32 unit roundoff


def sigmoid(v):
    return np.where(v >= 0, 1 / (1 + np.exp(-np.abs(v))), np.exp(-np.abs(v)) / (1 + np.exp(-np.abs(v)))).astype(v.dtype)


def act(v, name):
    if name in (None, "identity"):
        return v
    if name == "relu":
        return np.maximum(v, 0)
    if name == "softplus":
        return (np.log1p(np.exp(-np.abs(v))) + np.maximum(v, 0)).astype(v.dtype)
    if name == "tanh":
        return np.tanh(v)
    return v * sigmoid(v)      # swish


def dact(v, name):
    if name in (None, "identity"):
        return np.ones_like(v)
    if name == "relu":
        return (v > 0).astype(v.dtype)
    if name == "softplus":
        return sigmoid(v)
    if name == "tanh":
        return (1 - np.tanh(v)) * (1 + np.tanh(v))
    sg = sigmoid(v)
    return sg * (1 + v * (1 - sg))


def split_nonfinite(got, ref):
    """(got, ref, ok) with the reference's non-finite entries — the ∓Inf of a row without in-edges under max / min, NNlib's identity
    of an empty scatter, and what it turns into downstream — set to 0 in both; ok: got has exactly those values there (NaN for NaN)"""
    got, ref = np.asarray(got, f64), np.asarray(ref, f64)
    bad = ~np.isfinite(ref)
    if not bad.any():
        return got, ref, True
    return np.where(bad, 0.0, got), np.where(bad, 0.0, ref), bool(np.array_equal(got[bad], ref[bad], equal_nan=True))


def rel(got, ref):
    """norm-wise relative distance over the reference's finite entries; inf when the non-finite ones are not reproduced exactly"""
    got, ref, ok = split_nonfinite(got, ref)
    if not ok:
        return float("inf")
    return float(np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-300))


def seg_sum(idx, vals, n):
    """Σ over the rows of vals that share idx, in row order, in vals' dtype"""
    out = np.zeros((n,) + vals.shape[1:], vals.dtype)
    np.add.at(out, idx, vals)
    return out


# ---- the three exports ----------------------------------------------------------------------------------------------------------------
def edge(s, t, P, Q, F, name):
    """(a0, z0) of gnnmp_megnet_edge_f32"""
    z = P[t] + Q[s]
    if F is not None:
        z = z + F
    return act(z, name), z


def edge_grad(s, t, n, da0, z, name):
    """(dz0, dP, dQ) of gnnmp_megnet_edge_grad_f32"""
    dz = da0 if name == "identity" else da0 * dact(z, name)
    return dz, seg_sum(t, dz, n), seg_sum(s, dz, n)


def aggregate(t, n, m, aggr):
    """aggregate_neighbors(g, aggr, m); rows without in-edges: 0 for + and mean, NNlib's -Inf / +Inf for max / min"""
    if aggr in ("+", "mean"):
        y = seg_sum(t, m, n)
        if aggr == "mean":
            y = y / np.maximum(np.bincount(t, minlength=n), 1).astype(m.dtype)[:, None]
        return y.astype(m.dtype)
    y = np.full((n, m.shape[1]), -np.inf if aggr == "max" else np.inf, m.dtype)
    (np.maximum if aggr == "max" else np.minimum).at(y, t, m)
    return y


def aggregate_grad(t, n, dy, m, y, aggr, acc=None):
    """dm of gnnmp_aggregate_grad_f32"""
    if aggr == "+":
        term = dy[t]
    elif aggr == "mean":
        term = (dy / np.maximum(np.bincount(t, minlength=n), 1).astype(dy.dtype)[:, None])[t]
    else:
        term = np.where(m == y[t], dy[t], 0).astype(dy.dtype)
    return term if acc is None else acc + term


# ---- the layer -------------------------------------------------------------------------------------------------------------------------
def _inf_is_data(fn):
    """∓Inf rows (an empty max / min aggregation) are data here: Inf − Inf and 0 · Inf give the NaN the reference gives, without a warning"""
    def wrapped(*a, **kw):
        with np.errstate(invalid="ignore"):
            return fn(*a, **kw)
    wrapped.__doc__ = fn.__doc__
    return wrapped


@_inf_is_data
def forward(s, t, n, x, e, phi_e, phi_v, aggr, keep=None):
    """(x̄, ē) in the operands' dtype; phi_e / phi_v = [(W, b | None, act), ...].  The first ϕe layer is summed as the exports do:
    (P_i + Q_j) + F_k with the bias inside P.  keep (a dict) receives what the gradient reads"""
    nin = x.shape[1]
    W0, b0, a0n = phi_e[0]
    P = x @ W0[:, :nin].T + (0 if b0 is None else b0)
    Q = x @ W0[:, nin:2 * nin].T
    F = e @ W0[:, 2 * nin:].T
    h, z0 = edge(s, t, P, Q, F, a0n)
    pre_e, inp_e = [z0], [None]
    for W, b, a in phi_e[1:]:
        inp_e.append(h)
        z = h @ W.T + (0 if b is None else b)
        pre_e.append(z)
        h = act(z, a)
    eb = h
    xe = aggregate(t, n, eb, aggr)
    Wv, bv, av = phi_v[0]
    z = x @ Wv[:, :nin].T + xe @ Wv[:, nin:].T + (0 if bv is None else bv)
    pre_v, inp_v = [z], [None]
    h = act(z, av)
    for W, b, a in phi_v[1:]:
        inp_v.append(h)
        z = h @ W.T + (0 if b is None else b)
        pre_v.append(z)
        h = act(z, a)
    if keep is not None:
        keep.update(pre_e=pre_e, inp_e=inp_e, pre_v=pre_v, inp_v=inp_v, eb=eb, xe=xe)
    return h, eb


def _wgrad(dz, inp):
    """(dW, Σ|terms| of dW, db, Σ|terms| of db)"""
    return dz.T @ inp, np.abs(dz).T @ np.abs(inp), dz.sum(0), np.abs(dz).sum(0)


@_inf_is_data
def grad(s, t, n, x, e, phi_e, phi_v, aggr, dxb, deb):
    """the hand-derived pullback of forward for the loss Σ x̄ ⊙ dxb + Σ ē ⊙ deb (None: that output does not reach the loss).
    dict(xb, eb, dx, de, phi_e = [(dW, db | None)], phi_v likewise, mag_e, mag_v = [(Σ|terms| of dW, of db)], n_e, n_v = the n of the
    summation bound γ_n Σ|terms|).  THE CHOICE OF n: ϕe's gradients are sums over the E edge rows, n = E.  ϕv's are sums over the N node
    rows, but their terms are not exact inputs: ϕv's first layer reads xᵉ, itself a fold of up to E edge rows, so every term carries an
    E-row sum's rounding and γ_N — which bounds a sum of N EXACT products — does not bound a correctly rounded evaluation.  γ_n grows
    with n, so n = E, the longest fold on the path, serves both chains."""
    k = {}
    xb, eb = forward(s, t, n, x, e, phi_e, phi_v, aggr, k)
    nin, E = x.shape[1], len(s)
    gv, mv = [None] * len(phi_v), [None] * len(phi_v)
    dx = np.zeros_like(x)
    dxe = None
    if dxb is not None:
        d = dxb
        for q in range(len(phi_v) - 1, 0, -1):
            W, b, a = phi_v[q]
            dz = d * dact(k["pre_v"][q], a)
            dW, mW, db, mb = _wgrad(dz, k["inp_v"][q])
            gv[q], mv[q] = (dW, db if b is not None else None), (mW, mb)
            d = dz @ W
        Wv, bv, av = phi_v[0]
        dz = d * dact(k["pre_v"][0], av)
        dW, mW, db, mb = _wgrad(dz, np.concatenate([x, k["xe"]], axis=1))
        gv[0], mv[0] = (dW, db if bv is not None else None), (mW, mb)
        dx = dx + dz @ Wv[:, :nin]
        dxe = dz @ Wv[:, nin:]
    d = np.zeros_like(eb) if deb is None else deb
    if dxe is not None:
        d = aggregate_grad(t, n, dxe, eb, k["xe"], aggr, None if deb is None else deb)
    ge, me = [None] * len(phi_e), [None] * len(phi_e)
    for q in range(len(phi_e) - 1, 0, -1):
        W, b, a = phi_e[q]
        dz = d * dact(k["pre_e"][q], a)
        dW, mW, db, mb = _wgrad(dz, k["inp_e"][q])
        ge[q], me[q] = (dW, db if b is not None else None), (mW, mb)
        d = dz @ W
    W0, b0, a0n = phi_e[0]
    dz0, dP, dQ = edge_grad(s, t, n, d, k["pre_e"][0], a0n)
    dW, mW, db, mb = _wgrad(dz0, np.concatenate([x[t], x[s], e], axis=1))      # [dA | dB | dD] as the E-row sums they are
    ge[0], me[0] = (dW, db if b0 is not None else None), (mW, mb)
    dx = dx + dP @ W0[:, :nin] + dQ @ W0[:, nin:2 * nin]
    de = dz0 @ W0[:, 2 * nin:]
    return dict(xb=xb, eb=eb, dx=dx, de=de, phi_e=ge, phi_v=gv, mag_e=me, mag_v=mv, n_e=E, n_v=E, pre_e=k["pre_e"], pre_v=k["pre_v"],
                xe=k["xe"])


def gamma(n):
    """γ_n = n u / (1 − n u): |fl(Σ_{r < n} a_r b_r) − Σ a_r b_r| <= γ_n Σ |a_r b_r| in any order of summation (Higham, Accuracy and
    Stability of Numerical Algorithms, §3.1), u = 2^-24"""
    return n * U32 / (1 - n * U32)


# ---- the graph of the GPU tests --------------------------------------------------------------------------------------------------------
N_NODES, HUB = 40, 600
NO_IN, NO_OUT, HUB_NODE = 3, 5, 7


def graph():
    """(s, t, (k1, k2)) 0-based int64 on 40 nodes, 1330 edges, shuffled: 8 self loops, edges k1 and k2 the same pair j -> i (the cases
    give them identical feature rows: an exact tie), node 3 without in-edges, node 5 without out-edges, node 7 with 600 edges in and
    600 out"""
    rng = np.random.default_rng(23)
    n = N_NODES
    srcs, dsts = np.setdiff1d(np.arange(n), [NO_OUT]), np.setdiff1d(np.arange(n), [NO_IN])
    both = np.setdiff1d(np.arange(n), [NO_IN, NO_OUT, HUB_NODE])
    s, t = rng.choice(srcs, 130), rng.choice(dsts, 130)
    s[:8] = t[:8] = rng.choice(both, 8, replace=False)
    s[9], t[9] = s[8], t[8] = 11, 13                             # the repeated edge
    s = np.concatenate([s, rng.choice(srcs, HUB), np.full(HUB, HUB_NODE)])
    t = np.concatenate([t, np.full(HUB, HUB_NODE), rng.choice(dsts, HUB)])
    perm = rng.permutation(len(s))
    inv = np.argsort(perm)
    return s[perm].astype(np.int64), t[perm].astype(np.int64), (int(inv[8]), int(inv[9]))


def assert_graph(s, t, tie):
    n = N_NODES
    indeg, outdeg = np.bincount(t, minlength=n), np.bincount(s, minlength=n)
    assert len(s) == 1330 and s.min() >= 0 and max(s.max(), t.max()) < n
    assert (s == t).sum() >= 8 and s[tie[0]] == s[tie[1]] and t[tie[0]] == t[tie[1]] and tie[0] != tie[1]
    assert indeg[NO_IN] == 0 and outdeg[NO_OUT] == 0 and indeg[HUB_NODE] >= HUB and outdeg[HUB_NODE] >= HUB


# ---- the kernel-level cases -------------------------------------------------------------------------------------------------------------
WIDTHS = (1, 2, 3, 6, 7, 64, 100, 260)      # 4- / 8- / 16-byte lanes, tails, a second feature tile


def edge_case(hid, name, seed=0):
    """(P, Q, F, da0) float32 on graph(); for relu F is moved so that every pre-activation, with and without F, is >= 0.03 from 0"""
    s, t, _ = graph()
    rng = np.random.default_rng([seed, hid, ACT_CODE[name], 1])
    n, E = N_NODES, len(s)
    P, Q = rng.standard_normal((n, hid)).astype(f32), rng.standard_normal((n, hid)).astype(f32)
    F, da0 = rng.standard_normal((E, hid)).astype(f32), rng.standard_normal((E, hid)).astype(f32)
    if name == "relu":
        # a channel has only n² distinct pair sums P_i + Q_j: P on the multiples of 1/8, Q on the odd multiples of 1/16 keep every one of
        # them >= 1/16 from 0 (the case without F); with F, the few sums that land within 0.05 of 0 are moved 0.1 further out
        P, Q = (np.round(P * 8) / 8).astype(f32), (np.round(Q * 8) / 8 + 0.0625).astype(f32)
        z = (P[t] + Q[s]) + F
        F = np.where(np.abs(z) < 0.05, F + np.where(z >= 0, f32(0.1), f32(-0.1)), F).astype(f32)
    return P, Q, F, da0


def edge_ref64(hid, name, with_F, seed=0):
    """(a0, z0, dz0, dP, dQ) in float64 for edge_case"""
    s, t, _ = graph()
    P, Q, F, da0 = [a.astype(f64) for a in edge_case(hid, name, seed)]
    a0, z0 = edge(s, t, P, Q, F if with_F else None, name)
    return (a0, z0) + edge_grad(s, t, N_NODES, da0, z0, name)


def edge_condition(hid, name, with_F, seed=0):
    """(worst norm-wise distance of the float32 restatement from float64 over a0, z0, dz0, dP, dQ; the smallest |z0|)"""
    s, t, _ = graph()
    P, Q, F, da0 = edge_case(hid, name, seed)
    a0, z0 = edge(s, t, P, Q, F if with_F else None, name)
    got = (a0, z0) + edge_grad(s, t, N_NODES, da0, z0, name)
    ref = edge_ref64(hid, name, with_F, seed)
    return max(rel(g, r) for g, r in zip(got, ref)), float(np.abs(ref[1]).min())


def aggr_case(D, aggr, seed=0):
    """(dy, m, y, acc) float32 on graph().  m: the tied edges carry one row; under max / min the winner of every row and channel is
    moved 0.01 past the runner-up, and in channel 0 the tied pair IS the winner of its row.  y = aggregate(m) (exact for max / min)"""
    s, t, (k1, k2) = graph()
    rng = np.random.default_rng([seed, D, AGGR_CODE[aggr], 2])
    n, E = N_NODES, len(s)
    dy, acc = rng.standard_normal((n, D)).astype(f32), rng.standard_normal((E, D)).astype(f32)
    m = rng.standard_normal((E, D)).astype(f32)
    sign = f32(-1.0) if aggr == "min" else f32(1.0)
    m = m * sign                                   # build for max, flip back for min
    m[k2] = m[k1]
    cols = np.arange(D)
    for r in range(n):
        idx = np.flatnonzero((t == r) & (np.arange(E) != k2))
        if len(idx):
            w = idx[np.argmax(m[idx], axis=0)]
            m[w, cols] += f32(0.01)
    m[k1, 0] = m[t == t[k1], 0].max() + f32(1.0)
    m[k2] = m[k1]
    m = (m * sign).astype(f32)
    return dy, m, aggregate(t, n, m, aggr), acc


def aggr_ref64(D, aggr, with_acc, seed=0):
    s, t, _ = graph()
    dy, m, y, acc = [a.astype(f64) for a in aggr_case(D, aggr, seed)]
    return aggregate_grad(t, N_NODES, dy, m, y, aggr, acc if with_acc else None)


def margin(t, n, m, aggr, skip=None):
    """the smallest lead of a row-and-channel's winner over its runner-up (rows of two or more edges; edge `skip` left out)"""
    worst = np.inf
    for r in range(n):
        idx = np.flatnonzero(t == r)
        idx = idx[idx != skip] if skip is not None else idx
        if len(idx) >= 2:
            v = np.sort(m[idx] if aggr == "max" else -m[idx], axis=0)
            worst = min(worst, float((v[-1] - v[-2]).min()))
    return worst


def aggr_condition(D, aggr, with_acc, seed=0):
    """(distance of the float32 restatement from float64, the smallest winner's lead — inf for + and mean)"""
    s, t, (k1, k2) = graph()
    dy, m, y, acc = aggr_case(D, aggr, seed)
    got = aggregate_grad(t, N_NODES, dy, m, y, aggr, acc if with_acc else None)
    lead = margin(t, N_NODES, m.astype(f64), aggr, skip=k2) if aggr in ("max", "min") else np.inf
    return rel(got, aggr_ref64(D, aggr, with_acc, seed)), lead


# ---- the layer-level cases --------------------------------------------------------------------------------------------------------------
LAYER_SHAPES = ((12, 16), (7, 5), (32, 32))      # (in, out); e has `in` features as MEGNetConv(in => out) builds it
MODES = ("x", "e", "both")                        # which output reaches the loss
SCALE = 64.0      # x and e ~ N(0, 64²): 1e-3 is then a small part of a pre-activation's spread, so a seed can keep all 42 000 of them away
# find_seed(...): the first seed from 0 whose operands meet layer_condition (0 where not listed)
LAYER_SEEDS = {((7, 5), "max"): 1, ((7, 5), "min"): 4, ((32, 32), "+"): 1, ((32, 32), "mean"): 1, ((32, 32), "max"): 1, ((32, 32), "min"): 1}


def glorot(rng, rows_, cols, dtype=f32):
    lim = np.sqrt(6.0 / (rows_ + cols))
    return rng.uniform(-lim, lim, (rows_, cols)).astype(dtype)


def layer_case(shape, aggr, seed=None, act0="relu", bias=True):
    """(x, e, phi_e, phi_v, dxb, deb) float32 on graph(), the default chains Dense(3 in => out, act0), Dense(out => out) and
    Dense(in + out => out, relu), Dense(out => out); the tied edges carry one e row"""
    if seed is None:
        seed = LAYER_SEEDS.get((shape, aggr), 0)
    s, t, (k1, k2) = graph()
    nin, out = shape
    rng = np.random.default_rng([seed, nin, out, 3])
    n, E = N_NODES, len(s)
    x = (SCALE * rng.standard_normal((n, nin))).astype(f32)
    e = (SCALE * rng.standard_normal((E, nin))).astype(f32)
    e[k2] = e[k1]
    b = lambda k: (SCALE * 0.1 * rng.standard_normal(k)).astype(f32) if bias else None      # noqa: E731
    phi_e = [(glorot(rng, out, 3 * nin), b(out), act0), (glorot(rng, out, out), b(out), None)]
    phi_v = [(glorot(rng, out, nin + out), b(out), "relu"), (glorot(rng, out, out), b(out), None)]
    dxb, deb = rng.standard_normal((n, out)).astype(f32), rng.standard_normal((E, out)).astype(f32)
    return x, e, phi_e, phi_v, dxb, deb


def _cast(case, dtype):
    x, e, phi_e, phi_v, dxb, deb = case
    c = lambda ch: [(W.astype(dtype), None if b is None else b.astype(dtype), a) for W, b, a in ch]      # noqa: E731
    return x.astype(dtype), e.astype(dtype), c(phi_e), c(phi_v), dxb.astype(dtype), deb.astype(dtype)


_REF = {}


def layer_ref64(shape, aggr, mode, seed=None):
    """grad(...) in float64 for layer_case, computed once per case and shared"""
    key = (shape, aggr, mode, seed)
    if key not in _REF:
        s, t, _ = graph()
        x, e, phi_e, phi_v, dxb, deb = _cast(layer_case(shape, aggr, seed), f64)
        _REF[key] = grad(s, t, N_NODES, x, e, phi_e, phi_v, aggr, dxb if mode in ("x", "both") else None, deb if mode in ("e", "both") else None)
    return _REF[key]


def layer_condition(shape, aggr, seed=None):
    """(worst norm-wise distance of the float32 restatement from float64 over x̄, ē, dx, de with both outputs in the loss; the smallest
    |pre-activation| of the relu layers; the smallest winner's lead of ē's rows under max / min — inf otherwise)"""
    s, t, (k1, k2) = graph()
    case = layer_case(shape, aggr, seed)
    ref = layer_ref64(shape, aggr, "both", seed)
    x, e, phi_e, phi_v, dxb, deb = case
    got = grad(s, t, N_NODES, x, e, phi_e, phi_v, aggr, dxb, deb)
    worst = max(rel(got[k], ref[k]) for k in ("xb", "eb", "dx", "de"))
    kink = min(float(np.abs(ref["pre_e"][0]).min()), float(np.abs(ref["pre_v"][0]).min()))
    lead = margin(t, N_NODES, ref["eb"], aggr, skip=k2) if aggr in ("max", "min") else np.inf
    return worst, kink, lead


def find_seed(shape, aggr, tries=200):
    for seed in range(tries):
        worst, kink, lead = layer_condition(shape, aggr, seed)
        if worst <= COND and kink >= KINK and lead >= KINK:
            return seed
    raise AssertionError((shape, aggr))


# ---- the finite-difference case -----------------------------------------------------------------------------------------------------------
def fd_case(name, aggr, bias, h):
    """a small graph (n = 7, E = 18, in = 3, ein = 2, hid = 4, out = 3) without repeated edges, every node with an in-edge; the first seed
    whose relu pre-activations and max / min leads are more than 100 h from their kinks"""
    n, E, nin, ein, hid, out = 7, 18, 3, 2, 4, 3
    for seed in range(200):
        rng = np.random.default_rng([seed, ACT_CODE[name], AGGR_CODE[aggr], int(bias), 4])
        pairs = rng.permutation(n * n)[:E]
        s, t = (pairs // n).astype(np.int64), (pairs % n).astype(np.int64)
        x, e = rng.standard_normal((n, nin)), rng.standard_normal((E, ein))
        b = lambda k: 0.3 * rng.standard_normal(k) if bias else None      # noqa: E731
        phi_e = [(glorot(rng, hid, 2 * nin + ein, f64), b(hid), name), (glorot(rng, out, hid, f64), b(out), None)]
        phi_v = [(glorot(rng, hid, nin + out, f64), b(hid), "relu"), (glorot(rng, out, hid, f64), b(out), None)]
        dxb, deb = rng.standard_normal((n, out)), rng.standard_normal((E, out))
        k = {}
        forward(s, t, n, x, e, phi_e, phi_v, aggr, k)
        kinks = [np.abs(k["pre_v"][0]).min()] + ([np.abs(k["pre_e"][0]).min()] if name == "relu" else [])
        if aggr in ("max", "min"):
            kinks.append(margin(t, n, k["eb"], aggr))
        if min(kinks) > 100 * h and np.bincount(t, minlength=n).min() > 0:
            return s, t, n, x, e, phi_e, phi_v, dxb, deb
    raise AssertionError((name, aggr, bias))


MEGNET = dict(pts=256, radius=0.22, nin=8, hid=16, centers=8, seed=5)
