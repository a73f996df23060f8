"""A float64 numpy model of the gated layers' training path (tests/test_gated_conv_ad.py): Flux's GRU cell as gnnmp_gru_pointwise_f32
computes it and its pullback as include/gnnmp.h states gnnmp_gru_pointwise_grad_f32; GatedGraphConv (gated_graph_conv,
GNNlib/src/layers/conv.jl:218-233: per layer m = W_i h, the fold of m over the in-edges, h = GRU(fold, h)) for +, mean, max, min; and
ResGatedGraphConv (res_gated_graph_conv, conv.jl:287-300: σ.(U x_i + Σ_j sigmoid.(A x_i + B x_j) .* V x_j + bias)), with gradients derived
by hand.  Every function works in the dtype of its operands: the same text is the float32 restatement the input conditions use.
Edge k: s[k] -> t[k], 0-based.  max / min pullback: Δ where m_j == y_i, every tying copy included (NNlib's rule)."""
import numpy as np

import megnet_conv_ref as M

f32, f64 = np.float32, np.float64
COND, KINK = M.COND, M.KINK
rel, gamma, seg_sum, sigmoid, glorot = M.rel, M.gamma, M.seg_sum, M.sigmoid, M.glorot
AGGRS = M.AGGRS


# ---- the GRU cell and its pullback --------------------------------------------------------------------------------------------------------
def gru(gx, gh, b, h):
    """(h', r, z, h~): gates r, z, candidate of gx + gh (+ b); h' = (1 - z) h~ + z h"""
    D = h.shape[1]
    bb = np.zeros(3 * D, h.dtype) if b is None else b
    r = sigmoid(gx[:, :D] + gh[:, :D] + bb[:D])
    z = sigmoid(gx[:, D:2 * D] + gh[:, D:2 * D] + bb[D:2 * D])
    c = np.tanh(gx[:, 2 * D:] + r * gh[:, 2 * D:] + bb[2 * D:])
    return (1 - z) * c + z * h, r, z, c


def gru_grad(gx, gh, b, h, dout, base=None):
    """(dgx, dgh, dh) of gnnmp_gru_pointwise_grad_f32"""
    D = h.shape[1]
    _, r, z, c = gru(gx, gh, b, h)
    dh = dout * z
    dz = (dout * (h - c)) * (z * (1 - z))
    dn = (dout * (1 - z)) * (1 - c * c)
    dr = (dn * gh[:, 2 * D:]) * (r * (1 - r))
    return np.concatenate([dr, dz, dn], 1), np.concatenate([dr, dz, dn * r], 1), dh if base is None else base + dh


GRU_DS = (1, 2, 3, 4, 5, 8, 33, 130)      # one thread an element: D from 1 across every tail of a 4-wide vector and of a wave
GRU_N = 37


def gru_case(D, seed=0):
    """(gx, gh, b, h, dout, base) float32"""
    rng = np.random.default_rng([seed, D, 31])
    nrm = lambda *sh: rng.standard_normal(sh).astype(f32)      # noqa: E731
    return nrm(GRU_N, 3 * D), nrm(GRU_N, 3 * D), nrm(3 * D), nrm(GRU_N, D), nrm(GRU_N, D), nrm(GRU_N, D)


def gru_ref(D, with_b, with_base, seed=0, dtype=f64):
    gx, gh, b, h, dout, base = [a.astype(dtype) for a in gru_case(D, seed)]
    return gru_grad(gx, gh, b if with_b else None, h, dout, base if with_base else None)


def gru_condition(D, with_b, with_base, seed=0):
    return max(rel(g, r) for g, r in zip(gru_ref(D, with_b, with_base, seed, f32), gru_ref(D, with_b, with_base, seed, f64)))


# ---- the fold -----------------------------------------------------------------------------------------------------------------------------
def fold(s, t, n, m, aggr):
    """propagate(copy_xj, g, aggr; xj = m)"""
    return M.aggregate(t, n, m[s], aggr)


def fold_grad(s, t, n, dy, m, y, aggr):
    """Δm [n][D] of fold"""
    return seg_sum(s, M.aggregate_grad(t, n, dy, m[s], y, aggr), n)


# ---- GatedGraphConv -------------------------------------------------------------------------------------------------------------------------
def ggc_forward(s, t, n, x, W, Wi, Wh, b, aggr, keep=None):
    """h [n][dims]; W [layers][dims][dims], Wi, Wh [3 dims][dims], b [3 dims]"""
    dims = W.shape[1]
    h = np.concatenate([x, np.zeros((n, dims - x.shape[1]), x.dtype)], 1)
    tape = []
    for Wl in W:
        m = h @ Wl.T
        a = fold(s, t, n, m, aggr)
        gx, gh = a @ Wi.T, h @ Wh.T
        tape.append((h, m, a, gx, gh))
        h = gru(gx, gh, b, h)[0]
    if keep is not None:
        keep["tape"] = tape
    return h


def ggc_grad(s, t, n, x, W, Wi, Wh, b, aggr, dY):
    """dict(Y, dx, dW, dWi, dWh, db and the Σ|terms| of each weight gradient, mag_*) for the loss Σ Y ⊙ dY"""
    keep = {}
    Y = ggc_forward(s, t, n, x, W, Wi, Wh, b, aggr, keep)
    dW, mW = np.zeros_like(W), np.zeros_like(W)
    dWi, dWh, db = np.zeros_like(Wi), np.zeros_like(Wh), np.zeros_like(b)
    mWi, mWh, mb = np.zeros_like(Wi), np.zeros_like(Wh), np.zeros_like(b)
    d = dY
    for q in range(len(W) - 1, -1, -1):
        h, m, a, gx, gh = keep["tape"][q]
        dgx, dgh, dh = gru_grad(gx, gh, b, h, d)
        dWi, mWi = dWi + dgx.T @ a, mWi + np.abs(dgx).T @ np.abs(a)
        dWh, mWh = dWh + dgh.T @ h, mWh + np.abs(dgh).T @ np.abs(h)
        db, mb = db + dgx.sum(0), mb + np.abs(dgx).sum(0)
        dm = fold_grad(s, t, n, dgx @ Wi, m, a, aggr)
        dW[q], mW[q] = dm.T @ h, np.abs(dm).T @ np.abs(h)
        d = dh + dgh @ Wh + dm @ W[q]
    return dict(Y=Y, dx=d[:, :x.shape[1]], dW=dW, dWi=dWi, dWh=dWh, db=db, mag_W=mW, mag_Wi=mWi, mag_Wh=mWh, mag_b=mb, tape=keep["tape"])


# ---- ResGatedGraphConv ----------------------------------------------------------------------------------------------------------------------
def rgc_forward(s, t, n, x, A, B, U, V, bias, sigma, keep=None):
    Ax, Bx, Vx = x @ A.T, x @ B.T, x @ V.T
    gate = sigmoid(Ax[t] + Bx[s])
    pre = x @ U.T + seg_sum(t, gate * Vx[s], n)
    if bias is not None:
        pre = pre + bias
    if keep is not None:
        keep.update(gate=gate, Vx=Vx, pre=pre)
    return M.act(pre, sigma)


def rgc_grad(s, t, n, x, A, B, U, V, bias, sigma, dY):
    """dict(Y, dx, dA, dB, dU, dV, db, mag_*)"""
    k = {}
    Y = rgc_forward(s, t, n, x, A, B, U, V, bias, sigma, k)
    gate, Vx = k["gate"], k["Vx"]
    dz = dY * M.dact(k["pre"], sigma)
    dmsg = dz[t]
    dgate = dmsg * Vx[s] * gate * (1 - gate)
    dAx, dBx, dVx = seg_sum(t, dgate, n), seg_sum(s, dgate, n), seg_sum(s, dmsg * gate, n)
    ax = np.abs(x)
    return dict(Y=Y, pre=k["pre"], dx=dz @ U + dAx @ A + dBx @ B + dVx @ V, dA=dAx.T @ x, dB=dBx.T @ x, dU=dz.T @ x, dV=dVx.T @ x, db=dz.sum(0),
                mag_A=np.abs(dAx).T @ ax, mag_B=np.abs(dBx).T @ ax, mag_U=np.abs(dz).T @ ax, mag_V=np.abs(dVx).T @ ax, mag_b=np.abs(dz).sum(0))


# ---- the layer cases ------------------------------------------------------------------------------------------------------------------------
N_NODES, N_EDGES = 24, 72


def layer_graph():
    """(s, t, (k1, k2)) 0-based on 24 nodes, 72 edges, shuffled: a ring (every node has an in-edge and an out-edge: max / min stay
    finite), random extras, two self loops, and edges k1, k2 the same pair j -> i: under max / min their messages tie EXACTLY"""
    rng = np.random.default_rng(41)
    n = N_NODES
    s = np.concatenate([np.arange(n), rng.integers(0, n, N_EDGES - n)])
    t = np.concatenate([(np.arange(n) + 1) % n, rng.integers(0, n, N_EDGES - n)])
    s[n], t[n] = 4, 4
    s[n + 1], t[n + 1] = 9, 9
    s[n + 3], t[n + 3] = s[n + 2], t[n + 2] = 2, 17
    perm = rng.permutation(N_EDGES)
    inv = np.argsort(perm)
    return s[perm].astype(np.int64), t[perm].astype(np.int64), (int(inv[n + 2]), int(inv[n + 3]))


GGC_CASES = [(aggr, m, layers) for aggr in AGGRS for m in (4, 6) for layers in (1, 3)]      # dims = 6: m < dims and m = dims
GGC_DIMS = 6
# the first seed from 0 whose operands meet ggc_condition (find_ggc_seed; 0 where not listed)
GGC_SEEDS = {("max", 4, 3): 88, ("max", 6, 1): 11, ("max", 6, 3): 81, ("min", 4, 1): 3, ("min", 4, 3): 19, ("min", 6, 3): 241}
RGC_CASES = [(sigma, bias) for sigma in (None, "relu") for bias in (True, False)]
RGC_SHAPE = (7, 10)
RGC_SEEDS = {}


def ggc_case(aggr, m, layers, seed=None):
    """(x, W, Wi, Wh, b, dY) float32 on layer_graph()"""
    if seed is None:
        seed = GGC_SEEDS.get((aggr, m, layers), 0)
    dims = GGC_DIMS
    rng = np.random.default_rng([seed, AGGRS.index(aggr), m, layers, 32])
    x = rng.standard_normal((N_NODES, m)).astype(f32)
    W = np.stack([glorot(rng, dims, dims) for _ in range(layers)])
    Wi, Wh = glorot(rng, 3 * dims, dims), glorot(rng, 3 * dims, dims)
    b = (0.1 * rng.standard_normal(3 * dims)).astype(f32)
    return x, W, Wi, Wh, b, rng.standard_normal((N_NODES, dims)).astype(f32)


_REF = {}


def ggc_ref(aggr, m, layers, seed=None, dtype=f64):
    key = ("ggc", aggr, m, layers, seed, dtype)
    if key not in _REF:
        s, t, _ = layer_graph()
        _REF[key] = ggc_grad(s, t, N_NODES, *[a.astype(dtype) for a in ggc_case(aggr, m, layers, seed)][:5], aggr,
                             ggc_case(aggr, m, layers, seed)[5].astype(dtype))
    return _REF[key]


def ggc_condition(aggr, m, layers, seed=None):
    """(worst norm-wise distance of the float32 restatement from float64 over Y, dx and the four weight gradients; under max / min the
    smallest lead of a row-and-channel's winner over its runner-up over every layer, the tied copy k2 left out — inf for + and mean)"""
    s, t, (k1, k2) = layer_graph()
    got, ref = ggc_ref(aggr, m, layers, seed, f32), ggc_ref(aggr, m, layers, seed, f64)
    worst = max(rel(got[q], ref[q]) for q in ("Y", "dx", "dW", "dWi", "dWh", "db"))
    lead = np.inf
    if aggr in ("max", "min"):
        lead = min(M.margin(t, N_NODES, mm[s], aggr, skip=k2) for _, mm, *_ in ref["tape"])
    return worst, lead


def find_ggc_seed(aggr, m, layers, tries=2000):
    for seed in range(tries):
        worst, lead = ggc_condition(aggr, m, layers, seed)
        if worst <= COND and lead >= KINK:
            return seed
    raise AssertionError((aggr, m, layers))


def rgc_case(sigma, bias, seed=None):
    """(x, A, B, U, V, bias, dY) float32 on layer_graph()"""
    if seed is None:
        seed = RGC_SEEDS.get((sigma, bias), 0)
    nin, out = RGC_SHAPE
    rng = np.random.default_rng([seed, int(sigma == "relu"), int(bias), 33])
    x = rng.standard_normal((N_NODES, nin)).astype(f32)
    A, B, U, V = (glorot(rng, out, nin) for _ in range(4))
    bv = (0.1 * rng.standard_normal(out)).astype(f32) if bias else None
    return x, A, B, U, V, bv, rng.standard_normal((N_NODES, out)).astype(f32)


def rgc_ref(sigma, bias, seed=None, dtype=f64):
    key = ("rgc", sigma, bias, seed, dtype)
    if key not in _REF:
        s, t, _ = layer_graph()
        c = [None if a is None else a.astype(dtype) for a in rgc_case(sigma, bias, seed)]
        _REF[key] = rgc_grad(s, t, N_NODES, *c[:6], sigma, c[6])
    return _REF[key]


def rgc_condition(sigma, bias, seed=None):
    """(distance of the float32 restatement from float64; the smallest |pre-activation| under relu — inf for identity)"""
    got, ref = rgc_ref(sigma, bias, seed, f32), rgc_ref(sigma, bias, seed, f64)
    worst = max(rel(got[q], ref[q]) for q in ("Y", "dx", "dA", "dB", "dU", "dV", "db"))
    return worst, float(np.abs(ref["pre"]).min()) if sigma == "relu" else np.inf


def find_rgc_seed(sigma, bias, tries=200):
    for seed in range(tries):
        worst, kink = rgc_condition(sigma, bias, seed)
        if worst <= COND and kink >= KINK:
            return seed
    raise AssertionError((sigma, bias))


def sum_n(n_nodes, n_edges, width, layers):
    """THE n OF THE WEIGHT GRADIENTS' BOUND γ_n Σ|terms|.  A weight gradient is a sum over the N node rows, but its terms are not exact
    inputs: each reaches the sum through `layers` rounds of a dense product (width additions), a fold of at most E slots and a second
    dense product, forward and again backward.  To first order the roundings of a chain of sums add, so n = N + 2 layers (E + 2 width):
    the sum's own length plus every addition on the longest path from an input to one of its terms (the convention of
    tests/megnet_conv_ref.py: the longest fold on the path, here once per layer and direction)."""
    return n_nodes + 2 * layers * (n_edges + 2 * width)
