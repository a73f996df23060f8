"""numpy references of tests/test_edge_conv_ad.py — TEST INFRASTRUCTURE ONLY.

  * compose / grad64: the reference's own composition of EdgeConv with a one-layer nn (GNNlib/src/layers/conv.jl:237-246: the per-edge
    vcat(xi, xj - xi), the Dense on E rows, the scatter) restated in float64, and its pullback written by hand.  max / min hand Δ to EVERY
    maximiser (NNlib's rule: ∇scatter(max) = (src .== gather(dst)) .* gather(Δ)); torch's amax splits Δ among ties and is the wrong oracle.
  * stack_p / split_pre / fused / grad_p: the formulation of include/gnnmp.h (P = x [W1; W2]' + [b; 0] planar, a_i = P[i][c] - P[i][C+c],
    pre_e = a_i + P[j][C+c]) in the dtype of its operands, every fold a sequential loop in edge order — the bits the kernels owe when
    the operands are float32.
  * conditioning: how far the float32 split formulation is from the float64 composition, and how far the inputs keep from relu's kink and
    from a change of winner.
Edge indices are 0-based here."""
import numpy as np

f32, f64 = np.float32, np.float64
AGGRS = ("+", "mean", "max", "min")
ACTS = (None, "relu")
AGGR_CODE = {"+": 0, "mean": 1, "max": 2, "min": 3}
ACT_CODE = {None: 0, "relu": 1}


def act(v, sigma):
    return v if sigma is None else np.where(v < 0, v.dtype.type(0), v)      # NNlib.relu = ifelse(x < 0, zero(x), x)


def fold(t, n, m, aggr):
    """y[i] = aggr of m[e] over the edges into i, sequentially in edge order, in m's dtype; empty rows keep the identity"""
    init = {"+": 0.0, "mean": 0.0, "max": -np.inf, "min": np.inf}[aggr]
    y = np.full((n, m.shape[1]), init, m.dtype)
    op = {"+": np.add, "mean": np.add, "max": np.maximum, "min": np.minimum}[aggr]
    for e in range(len(t)):
        y[t[e]] = op(y[t[e]], m[e])
    if aggr == "mean":
        cnt = np.bincount(t, minlength=n)
        nz = cnt > 0
        y[nz] = y[nz] / cnt[nz, None].astype(m.dtype)                       # true division
    return y


# ---- the reference's composition, float64 -----------------------------------------------------------------------------------------
def compose(s, t, n, x, W, b, aggr, sigma):
    """(z, pre, m, y) of nn(vcat(xi, xj - xi)) per edge and its aggregation, float64"""
    x, W = np.asarray(x, f64), np.asarray(W, f64)
    z = np.concatenate([x[t], x[s] - x[t]], axis=1)
    pre = z @ W.T + (0.0 if b is None else np.asarray(b, f64))
    m = act(pre, sigma)
    return z, pre, m, fold(t, n, m, aggr)


def edge_g(t, n, pre, m, y, dy, aggr, sigma):
    """g_e [E][C]: what reaches pre_e of Δ = dy.  + : Δ_i; mean: Δ_i / count_i (divided once per row); max / min: Δ_i for EVERY edge whose
    message equals the row's extremum; relu' = (pre > 0)"""
    if aggr == "+":
        r = dy[t]
    elif aggr == "mean":
        cnt = np.bincount(t, minlength=n)
        r = (dy / np.maximum(cnt, 1)[:, None].astype(dy.dtype))[t]
    else:
        r = np.where(m == y[t], dy[t], dy.dtype.type(0))
    return r if sigma is None else np.where(pre > 0, r, dy.dtype.type(0))


def grad64(s, t, n, x, W, b, aggr, sigma, dy):
    """the composition and its hand-written pullback: dict(y, pre, m, g, dx, dW, db), float64"""
    z, pre, m, y = compose(s, t, n, x, W, b, aggr, sigma)
    g = edge_g(t, n, pre, m, y, np.asarray(dy, f64), aggr, sigma)
    D = np.asarray(x).shape[1]
    dz = g @ np.asarray(W, f64)
    dx = np.zeros((n, D), f64)
    np.add.at(dx, t, dz[:, :D] - dz[:, D:])
    np.add.at(dx, s, dz[:, D:])
    return dict(y=y, pre=pre, m=m, g=g, dx=dx, dW=g.T @ z, db=g.sum(axis=0))


# ---- the split formulation, in the operands' dtype ------------------------------------------------------------------------------------
def stack_p(x, W, b, dtype):
    """P [N][2C] planar: columns [0, C) = x W1' + b, columns [C, 2C) = x W2'"""
    x, W = np.asarray(x, dtype), np.asarray(W, dtype)
    D = x.shape[1]
    pi = x @ W[:, :D].T
    if b is not None:
        pi = pi + np.asarray(b, dtype)
    return np.ascontiguousarray(np.concatenate([pi, x @ W[:, D:].T], axis=1), dtype=dtype)


def split_pre(s, t, P, C):
    a = P[:, :C] - P[:, C:]
    return a[t] + P[s][:, C:]


def fused(s, t, n, P, C, aggr, sigma):
    """(y, pre, m) by the formulation of the header, in P's dtype"""
    pre = split_pre(s, t, P, C)
    m = act(pre, sigma)
    return fold(t, n, m, aggr), pre, m


def dp_from_g(s, t, n, g):
    """dP [N][2C] from the per-edge g: dA and dB summed sequentially in edge order, then dP[:, C:] = dB - dA"""
    C = g.shape[1]
    dA, dB = np.zeros((n, C), g.dtype), np.zeros((n, C), g.dtype)
    for e in range(len(t)):
        dA[t[e]] = dA[t[e]] + g[e]
        dB[s[e]] = dB[s[e]] + g[e]
    return np.concatenate([dA, dB - dA], axis=1)


def grad_p(s, t, n, P, C, y, dy, aggr, sigma):
    """dP of the header's backward in the dtype of P / dy (float32: the bits of the kernels), pre and m recomputed from P"""
    pre = split_pre(s, t, P, C)
    return dp_from_g(s, t, n, edge_g(t, n, pre, act(pre, sigma), y, dy, aggr, sigma))


# ---- conditioning ---------------------------------------------------------------------------------------------------------------------
def conditioning(s, t, n, x, W, b):
    """(dev, kink, gap): dev = max |pre_fp32split - pre_float64|; kink = the smallest |pre_e|; gap = the smallest top-two gap of m over
    all (row, channel) cells, for max and for min, with and without relu, whose extremum is not relu's exact 0"""
    x32, W32 = np.asarray(x, f32), np.asarray(W, f32)
    b32 = None if b is None else np.asarray(b, f32)
    pre64 = compose(s, t, n, x32, W32, b32, "+", None)[1]
    C = W32.shape[0]
    pre32 = split_pre(s, t, stack_p(x32, W32, b32, f32), C)
    dev = float(np.abs(pre32.astype(f64) - pre64).max())
    kink = float(np.abs(pre64).min())
    gap = np.inf
    order = np.argsort(t, kind="stable")
    bounds = np.searchsorted(t[order], np.arange(n + 1))
    for sigma in ACTS:
        m = act(pre64, sigma)
        for i in range(n):
            rows = m[order[bounds[i]:bounds[i + 1]]]
            if rows.shape[0] < 2:
                continue
            srt = np.sort(rows, axis=0)
            for ext, second in ((srt[-1], srt[-2]), (srt[0], srt[1])):
                d = np.abs(ext - second)
                keep = np.ones_like(d, bool) if sigma is None else ext != 0
                if keep.any():
                    gap = min(gap, float(d[keep].min()))
    return dev, kink, gap


def knn_cpu(x, k, gi):
    """(s, t) of knn_graph(x, k; graph_indicator = gi, dir = :in) by brute force in float64: edge i k + r joins node i (target) and its
    r-th nearest neighbour of the same graph (source), the node itself excluded"""
    x = np.asarray(x, f64)
    n = x.shape[0]
    s, t = [], []
    for i in range(n):
        d = ((x - x[i]) ** 2).sum(axis=1)
        d[gi != gi[i]] = np.inf
        d[i] = np.inf
        nb = np.argsort(d, kind="stable")[:k]
        s += list(nb)
        t += [i] * k
    return np.array(s, np.int64), np.array(t, np.int64)


# The Gaussian cases of the GPU tests: (clouds, points per cloud, D, k, C, seed).  The seeds were picked by searching on the CPU for inputs
# that keep float32 away from the discontinuities (tests/test_edge_conv_ad.py asserts the condition, on the CPU and again on the device's
# own graph).
GAUSSIAN = {"cond": (2, 128, 5, 6, 12, 4), "wide": (2, 32, 64, 8, 64, 8)}


def gaussian_case(name):
    """x [n][D] (the point coordinates ARE the features), graph indicator (0-based), k, W [C][2D] ~ 0.4 N(0,1), b ~ 0.2 N(0,1), Δ ~ N(0,1)"""
    clouds, pts, D, k, C, seed = GAUSSIAN[name]
    rng = np.random.default_rng(seed)
    n = clouds * pts
    x = rng.standard_normal((n, D)).astype(f32)
    W = (0.4 * rng.standard_normal((C, 2 * D))).astype(f32)
    b = (0.2 * rng.standard_normal(C)).astype(f32)
    dy = rng.standard_normal((n, C)).astype(f32)
    return x, np.repeat(np.arange(clouds), pts), k, W, b, dy


# The small DGCNN step: 4 clouds of 64 points in R^3, k = 6, C = 16 then 24, relu, max; global mean pool; loss = Σ pooled .* R
DGCNN = dict(clouds=4, pts=64, D=3, k=6, C=(16, 24), seed=7)


def dgcnn_case():
    c = DGCNN
    rng = np.random.default_rng(c["seed"])
    n = c["clouds"] * c["pts"]
    x = rng.standard_normal((n, c["D"])).astype(f32)
    dims = (c["D"],) + c["C"]
    Ws = [(0.4 * rng.standard_normal((dims[l + 1], 2 * dims[l]))).astype(f32) for l in range(2)]
    bs = [(0.2 * rng.standard_normal(dims[l + 1])).astype(f32) for l in range(2)]
    R = rng.standard_normal((c["clouds"], c["C"][1])).astype(f32)
    return x, np.repeat(np.arange(c["clouds"]), c["pts"]), c["k"], Ws, bs, R


def dgcnn_grad64(edges, gi, x, Ws, bs, R, aggr="max", sigma="relu"):
    """float64 gradients of loss = Σ mean_pool(h2) .* R through two EdgeConv layers on the given edge lists [(s1, t1), (s2, t2)]:
    (h1, h2, [(dW1, db1), (dW2, db2)], dx)"""
    n = x.shape[0]
    (s1, t1), (s2, t2) = edges
    h1 = compose(s1, t1, n, x, Ws[0], bs[0], aggr, sigma)[3]
    h2 = compose(s2, t2, n, h1, Ws[1], bs[1], aggr, sigma)[3]
    cnt = np.bincount(gi, minlength=R.shape[0])
    dh2 = (np.asarray(R, f64) / cnt[:, None])[gi]
    g2 = grad64(s2, t2, n, h1, Ws[1], bs[1], aggr, sigma, dh2)
    g1 = grad64(s1, t1, n, x, Ws[0], bs[0], aggr, sigma, g2["dx"])
    return h1, h2, [(g1["dW"], g1["db"]), (g2["dW"], g2["db"])], g1["dx"]
