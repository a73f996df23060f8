"""numpy references of tests/test_gmm_conv_ad.py — TEST INFRASTRUCTURE ONLY.

  * compose / grad64: GMMConv (GNNlib/src/layers/conv.jl:372-401: the mixture weights exp(+Σ ...), dense_x, the mean of w .* xj over the
    in-edges, the mean over the K kernels, bias, σ, the residual) in float64, and its pullback by the formulas of include/gnnmp.h.
  * weights / rows / rows_grad / wgrad / layer: the same formulas in the dtype of their operands, with the roundings of the header
    (products rounded, then added; every fold a sequential loop in edge order) — the float32 restatement the GPU cases are conditioned on.
  * the operands of every GPU case: e ~ U(-1, 1), mu and sigma_inv in glorot_uniform's range.
Edge indices are 0-based here.  The multigraph is the one of tests/cg_conv_ref.py."""
import functools

import numpy as np

import cg_conv_ref as CG

f32, f64 = np.float32, np.float64
ACTS = ("identity", "relu", "softplus", "tanh", "swish")
ACT_CODE = {"identity": 0, "relu": 1, "softplus": 2, "tanh": 3, "swish": 4}
COND = 2e-6         # a fifth of the project's 1e-5 bar
MARGIN = 20         # relu's kink is at least this many times farther away than float32 is from float64
PARTS = 256         # GNNMP_GMM_PARTS
N_NODES, N_EDGES = CG.N_NODES, 1500
graph, assert_graph = CG.graph, CG.assert_graph
sigmoid = CG.sigmoid


def act(v, name):
    if name == "swish":
        return v * sigmoid(v)
    return CG.act(v, name)


def dact(v, name):
    if name == "swish":
        sg = sigmoid(v)
        return sg * (v.dtype.type(1) + v * (v.dtype.type(1) - sg))
    return CG.dact(v, name)


def rel(got, ref):
    got, ref = np.asarray(got, f64), np.asarray(ref, f64)
    return float(np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-300))


# ---- the header's formulas in the operands' dtype ----------------------------------------------------------------------------------------
def weights(e, mu, sinv):
    """w [E][K] = exp(Σ_d ((e − mu)² / 2) sinv²), d ascending from 0, statement by statement as gmm_weights_kernel"""
    dt = e.dtype.type
    diff = e[:, None, :] - mu[None, :, :]
    term = ((diff * diff) / dt(2)) * (sinv * sinv)[None]
    a = np.zeros(term.shape[:2], e.dtype)
    for d in range(term.shape[2]):
        a = a + term[:, :, d]
    return np.exp(a)


def rows(s, t, n, w, xk, bias, K, C):
    """z [N][C] of gnnmp_gmm_conv_f32: the sequential fold in edge order, / deg, kernels in order, / K, + bias"""
    dt = xk.dtype.type
    acc = np.zeros((n, K, C), xk.dtype)
    xk3 = xk.reshape(n, K, C)
    for k in range(len(t)):
        acc[t[k]] = acc[t[k]] + w[k][:, None] * xk3[s[k]]
    deg = np.bincount(t, minlength=n)
    m = np.where(deg[:, None, None] > 0, acc / np.maximum(deg, 1).astype(xk.dtype)[:, None, None], acc)
    z = m[:, 0]
    for k in range(1, K):
        z = z + m[:, k]
    z = z / dt(K)
    return z if bias is None else z + bias[None, :]


def rows_grad(s, t, n, w, xk, dz, K, C):
    """(dxk [N][K C], dw [E][K]) of gnnmp_gmm_conv_grad_f32 (dw's sum over channels in plain ascending order)"""
    dt = xk.dtype.type
    deg = np.bincount(t, minlength=n)
    q = (dt(1) / (dt(K) * np.maximum(deg, 1).astype(xk.dtype)))
    tt = q[t][:, None] * dz[t]                                  # [E][C]
    xk3 = xk.reshape(n, K, C)
    dxk = np.zeros((n, K, C), xk.dtype)
    for k in range(len(t)):
        dxk[s[k]] = dxk[s[k]] + w[k][:, None] * tt[k][None, :]
    prod = xk3[s] * tt[:, None, :]                              # [E][K][C]
    dw = np.zeros((len(t), K), xk.dtype)
    for c in range(C):
        dw = dw + prod[:, :, c]
    return dxk.reshape(n, K * C), dw


def wgrad_terms(e, mu, sinv, w, dw):
    """per-edge terms of (de, dmu, dsinv): ([E][K][ein] each), rounded as the header says"""
    g = dw * w
    diff = e[:, None, :] - mu[None, :, :]
    gd = g[:, :, None] * diff
    t_e = gd * (sinv * sinv)[None]
    t_s = (g[:, :, None] * (diff * diff)) * sinv[None]
    return t_e, -t_e, t_s


def wgrad(e, mu, sinv, w, dw):
    """(de, dmu, dsinv) of gnnmp_gmm_weights_grad_f32 with plain sequential folds"""
    t_e, t_m, t_s = wgrad_terms(e, mu, sinv, w, dw)
    de = np.zeros(e.shape, e.dtype)
    for k in range(mu.shape[0]):
        de = de + t_e[:, k]
    dmu, dsinv = np.zeros(mu.shape, e.dtype), np.zeros(mu.shape, e.dtype)
    for i in range(len(e)):
        dmu, dsinv = dmu + t_m[i], dsinv + t_s[i]
    return de, dmu, dsinv


def wgrad64(e, mu, sinv, w, dw):
    """float64 on the given operands: (de, dmu, dsinv, Σ_e |term| of dmu, Σ_e |term| of dsinv)"""
    e, mu, sinv, w, dw = [np.asarray(a, f64) for a in (e, mu, sinv, w, dw)]
    t_e, t_m, t_s = wgrad_terms(e, mu, sinv, w, dw)
    return t_e.sum(axis=1), t_m.sum(axis=0), t_s.sum(axis=0), np.abs(t_m).sum(axis=0), np.abs(t_s).sum(axis=0)


def fold_depth(E):
    """the documented depth of the dmu / dsinv fold: slice length + GNNMP_GMM_PARTS"""
    return -(-E // PARTS) + PARTS


def sum_bound(E, mag):
    """the fp32 summation bound of tests/test_dense_fallbacks.py: (d + 8) 2^-24 Σ |term|"""
    return (fold_depth(E) + 8) * 2.0 ** -24 * np.asarray(mag, f64)


# ---- the layer -------------------------------------------------------------------------------------------------------------------------------
def layer(s, t, n, x, e, mu, sinv, W, bias, name, residual, dy, dtype=f64):
    """forward and pullback by the header's formulas in `dtype`: dict(w, xk, z, y, dz, dxk, dw, dx, de, dmu, dsinv, dW, db, mag_mu, mag_s)"""
    c = lambda a: None if a is None else np.asarray(a, dtype)      # noqa: E731
    x, e, mu, sinv, W, bias, dy = [c(a) for a in (x, e, mu, sinv, W, bias, dy)]
    K = mu.shape[0]
    C = W.shape[0] // K
    w = weights(e, mu, sinv)
    xk = x @ W.T
    z = rows(s, t, n, w, xk, bias, K, C)
    y = act(z, name)
    res = residual and x.shape[1] == C
    if res:
        y = y + x
    dz = dy * dact(z, name)
    dxk, dw = rows_grad(s, t, n, w, xk, dz, K, C)
    de, dmu, dsinv = wgrad(e, mu, sinv, w, dw)
    t_e, t_m, t_s = wgrad_terms(e, mu, sinv, w, dw)
    dx = dxk @ W
    if res:
        dx = dx + dy
    return dict(w=w, xk=xk, z=z, y=y, dz=dz, dxk=dxk, dw=dw, dx=dx, de=de, dmu=dmu, dsinv=dsinv, dW=dxk.T @ x, db=dz.sum(axis=0),
                mag_mu=np.abs(t_m).sum(axis=0), mag_s=np.abs(t_s).sum(axis=0))


def compose(s, t, n, x, e, mu, sinv, W, bias, name, residual):
    """the reference's own composition in float64, vectorised: (z, y)"""
    x, e, mu, sinv, W = [np.asarray(a, f64) for a in (x, e, mu, sinv, W)]
    K = mu.shape[0]
    C = W.shape[0] // K
    w = np.exp((((e[:, None, :] - mu[None]) ** 2 / 2) * (sinv ** 2)[None]).sum(axis=2))      # [E][K]
    xj = (x @ W.T).reshape(n, K, C)[s]
    m = np.zeros((n, K, C), f64)
    np.add.at(m, t, w[:, :, None] * xj)
    deg = np.bincount(t, minlength=n)
    m = m / np.maximum(deg, 1)[:, None, None]
    z = m.mean(axis=1) + (0.0 if bias is None else np.asarray(bias, f64))
    y = act(z, name)
    if residual and x.shape[1] == C:
        y = y + x
    return z, y


WHAT = ("y", "dx", "de", "dmu", "dsinv", "dW", "db")


# ---- operands ----------------------------------------------------------------------------------------------------------------------------------
def glorot(rng, rows_, cols, dtype=f32):
    sc = np.sqrt(6.0 / (rows_ + cols))
    return rng.uniform(-sc, sc, (rows_, cols)).astype(dtype)


KERNEL_CS = (1, 2, 3, 4, 5, 8, 33, 64, 130)
KERNEL_KS = (1, 2, 3, 4, 5, 16)
# every C with K = 3; every K (one per register capacity 1, 2, 3, 4, 8, 16) at one C per lane width: 5 (4-byte lanes), 130 (8-byte lanes,
# two tiles), 8 (16-byte lanes)
KERNEL_CASES = tuple((C, 3) for C in KERNEL_CS) + tuple((C, K) for C in (5, 130, 8) for K in KERNEL_KS if K != 3)
KERNEL_EIN = 3


@functools.lru_cache(maxsize=None)
def kernel_case(C, K, seed=0, with_bias=True):
    """(w [E][K], xk [N][K C], bias [C] | None, dz [N][C]) float32 on graph(); w from e ~ U(-1, 1), mu, sinv ~ glorot in float32"""
    rng = np.random.default_rng([seed, C, K])
    n, E = N_NODES, N_EDGES
    e = rng.uniform(-1, 1, (E, KERNEL_EIN)).astype(f32)
    mu, sinv = glorot(rng, K, KERNEL_EIN), glorot(rng, K, KERNEL_EIN)
    w = weights(e, mu, sinv)
    xk = rng.standard_normal((n, K * C)).astype(f32)
    bias = (0.2 * rng.standard_normal(C)).astype(f32) if with_bias else None
    dz = rng.standard_normal((n, C)).astype(f32)
    return w, xk, bias, dz


@functools.lru_cache(maxsize=None)
def kernel_ref64(C, K, seed=0, with_bias=True):
    """(z, dxk, dw) in float64 on the float32 operands of kernel_case"""
    s, t = graph()
    w, xk, bias, dz = [None if a is None else a.astype(f64) for a in kernel_case(C, K, seed, with_bias)]
    z = rows(s, t, N_NODES, w, xk, bias, K, C)
    dxk, dw = rows_grad(s, t, N_NODES, w, xk, dz, K, C)
    return z, dxk, dw


def kernel_condition(C, K):
    """the largest norm-wise distance of the float32 restatement of (z, dxk, dw) from float64"""
    s, t = graph()
    w, xk, bias, dz = kernel_case(C, K)
    z = rows(s, t, N_NODES, w, xk, bias, K, C)
    dxk, dw = rows_grad(s, t, N_NODES, w, xk, dz, K, C)
    return max(rel(g, r) for g, r in zip((z, dxk, dw), kernel_ref64(C, K)))


WGRAD_ES = (1, 7, 257, PARTS * 3 + 5)
WGRAD_CASES = tuple((E, ein, K) for E in WGRAD_ES for ein, K in ((3, 3), (1, 16), (2, 1), (5, 3)))


@functools.lru_cache(maxsize=None)
def wgrad_case(E, ein, K, seed=0):
    """(e, mu, sinv, w, dw) float32: w by the float32 formula, dw ~ N(0, 1)"""
    rng = np.random.default_rng([seed, E, ein, K])
    e = rng.uniform(-1, 1, (E, ein)).astype(f32)
    mu, sinv = glorot(rng, K, ein), glorot(rng, K, ein)
    return e, mu, sinv, weights(e, mu, sinv), rng.standard_normal((E, K)).astype(f32)


def wgrad_condition(E, ein, K):
    """(de's norm-wise distance float32 - float64; w's, against float64 weights of the same float32 operands; the worst
    |dmu, dsinv float32 − float64| / bound)"""
    e, mu, sinv, w, dw = wgrad_case(E, ein, K)
    de, dmu, dsinv = wgrad(e, mu, sinv, w, dw)
    de64, dmu64, dsinv64, mag_mu, mag_s = wgrad64(e, mu, sinv, w, dw)
    w64 = weights(e.astype(f64), mu.astype(f64), sinv.astype(f64))
    worst = max(float((np.abs(dmu - dmu64) / np.maximum(sum_bound(E, mag_mu), 1e-300)).max()),
                float((np.abs(dsinv - dsinv64) / np.maximum(sum_bound(E, mag_s), 1e-300)).max()))
    return rel(de, de64), rel(w, w64), worst


LAYER_SHAPES = {"applied": ((6, 3, 6), True), "not_applied": ((4, 2, 7), True), "off": ((6, 3, 6), False)}      # (nin, ein, out), residual
LAYER_KS = (1, 3)
LAYER_SEEDS = {}      # find_seed(...): the first seed from 0 whose operands meet layer_condition


@functools.lru_cache(maxsize=None)
def layer_case(shape, K, name, seed=None):
    """(x, e, mu, sinv, W, bias, Δ) float32 on graph(): x, Δ ~ N(0, 1), e ~ U(-1, 1), mu, sinv, W ~ glorot, bias ~ 0.2 N(0, 1)"""
    nin, ein, out = shape
    if seed is None:
        seed = LAYER_SEEDS.get((shape, K, name), 0)
    rng = np.random.default_rng([seed, nin, ein, out, K, ACT_CODE[name]])
    n, E = N_NODES, N_EDGES
    x = rng.standard_normal((n, nin)).astype(f32)
    e = rng.uniform(-1, 1, (E, ein)).astype(f32)
    mu, sinv = glorot(rng, K, ein), glorot(rng, K, ein)
    W = glorot(rng, K * out, nin)
    bias = (0.2 * rng.standard_normal(out)).astype(f32)
    dy = rng.standard_normal((n, out)).astype(f32)
    return x, e, mu, sinv, W, bias, dy


@functools.lru_cache(maxsize=None)
def layer_ref64(shape, K, name, residual, with_bias, seed=None):
    s, t = graph()
    x, e, mu, sinv, W, bias, dy = layer_case(shape, K, name, seed)
    return layer(s, t, N_NODES, x, e, mu, sinv, W, bias if with_bias else None, name, residual, dy, f64)


def layer_condition(shape, K, name, residual, with_bias, seed=None):
    """(worst norm-wise distance float32 - float64 over w, y, dx, de, dW, db; worst |dmu, dsinv float32 − float64| / bound; kink / dev)"""
    s, t = graph()
    x, e, mu, sinv, W, bias, dy = layer_case(shape, K, name, seed)
    got = layer(s, t, N_NODES, x, e, mu, sinv, W, bias if with_bias else None, name, residual, dy, f32)
    ref = layer_ref64(shape, K, name, residual, with_bias, seed)
    worst = max(rel(got[k], ref[k]) for k in ("w", "y", "dx", "de", "dW", "db"))
    E = len(e)
    summ = max(float((np.abs(got["dmu"] - ref["dmu"]) / np.maximum(sum_bound(E, ref["mag_mu"]), 1e-300)).max()),
               float((np.abs(got["dsinv"] - ref["dsinv"]) / np.maximum(sum_bound(E, ref["mag_s"]), 1e-300)).max()))
    dev = float(np.abs(got["z"].astype(f64) - ref["z"]).max())
    # a row without in-edges and without bias has z = 0 exactly, in every precision, and relu'(0) = 0 on both sides: not a kink to avoid
    live = np.abs(ref["z"])[(ref["z"] != 0) | (got["z"] != 0)]
    return worst, summ, float(live.min()) / max(dev, 2.0 ** -149)


def conditioned(cond, name):
    worst, summ, ratio = cond
    return worst <= COND and summ <= 0.2 and (name != "relu" or ratio >= MARGIN)


def find_seed(shape, K, name):
    """the search LAYER_SEEDS is filled by: the first seed from 0 on whose operands are well conditioned under every residual / bias"""
    for seed in range(1000):
        if all(conditioned(layer_condition(shape, K, name, r, b, seed), name) for r in (False, True) for b in (False, True)):
            return seed
    raise AssertionError(f"no well-conditioned seed for {shape} {K} {name}")


# ---- finite differences and the MoNet step -------------------------------------------------------------------------------------------------
def fd_case(nin, name, with_bias, seed=1):
    """n = 30, E = 200, ein = 3, K = 3, out = 5, float64: e ~ U(-1, 1), the rest U(-1, 1) scaled"""
    rng = np.random.default_rng([seed, nin, ACT_CODE[name], int(with_bias)])
    n, E, ein, K, C = 30, 200, 3, 3, 5
    s, t = rng.integers(0, n, E), rng.integers(0, n, E)
    u = lambda *shape: rng.uniform(-1, 1, shape)      # noqa: E731
    return (s, t, n, u(n, nin), u(E, ein), glorot(rng, K, ein, f64), glorot(rng, K, ein, f64), u(K * C, nin), u(C) if with_bias else None,
            u(n, C))


MONET = dict(clouds=4, pts=64, k=6, nin=8, hid=16, K=3, seed=3)
