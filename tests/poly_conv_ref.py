"""A float64 numpy model of the polynomial layers' training path (tests/test_poly_conv_ad.py): gnnmp_poly_hop_f32 as include/gnnmp.h
states it, ChebConv (cheb_conv, GNNlib/src/layers/conv.jl:83-98: Z_1 = X, Z_2 = L̃ Z_1, Z_k = 2 L̃ Z_{k-1} - Z_{k-2}, Y = Σ Z_k W_k' .+ b) and
DConv (d_conv, conv.jl:696-724: two diffusion directions, `T0` never advanced, weight slice 2 read twice) with their gradients derived by
hand.  Every function works in the dtype of its operands, so the same text is the float32 restatement the input conditions use.
Edge k: s[k] -> t[k], 0-based.  A plan's slot order is the stable sort by destination, so a row's slots are its edges in edge order and
the per-slot factors are given per EDGE here (w[k], ss[k])."""
import itertools

import numpy as np

import megnet_conv_ref as M

f32, f64 = np.float32, np.float64
COND, KINK, N_NODES, WIDTHS = M.COND, M.KINK, M.N_NODES, M.WIDTHS
rel, gamma, seg_sum, graph, assert_graph, glorot = M.rel, M.gamma, M.seg_sum, M.graph, M.assert_graph, M.glorot
NO_IN, NO_OUT = M.NO_IN, M.NO_OUT


# ---- the export ------------------------------------------------------------------------------------------------------------------------
def hop(s, t, n_dst, z, w=None, ss=None, sd=None, alpha=1.0, beta=0.0, self_=None, gam=0.0, prev=None, add=None):
    """out of gnnmp_poly_hop_f32 over the plan of (s, t), in the header's order of operations; the scalars are taken in z's dtype"""
    T = z.dtype.type
    m = z[s]
    if ss is not None:
        m = m * ss[:, None]
    if w is not None:
        m = w[:, None] * m
    r = seg_sum(t, m, n_dst)
    if sd is not None:
        r = r * sd[:, None]
    r = T(alpha) * r
    if self_ is not None:
        r = r + T(beta) * self_
    if prev is not None:
        r = r + T(gam) * prev
    if add is not None:
        r = r + add
    return r


FIELDS = ("w", "ss", "sd", "self_", "prev", "add")
COMBOS = list(itertools.product((False, True), repeat=len(FIELDS)))      # every combination of present / NULL
ALPHA, BETA, GAMMA = -0.75, 1.5, -1.25      # exact in float32


def hop_case(D, transposed, seed=0):
    """(s, t, operands) float32 on graph() — transposed: the reversed edge index, what the transposed plan walks"""
    s, t, _ = graph()
    if transposed:
        s, t = t, s
    rng = np.random.default_rng([seed, D, int(transposed), 11])
    n, E = N_NODES, len(s)
    nrm = lambda *sh: rng.standard_normal(sh).astype(f32)      # noqa: E731
    ops = dict(z=nrm(n, D), w=rng.uniform(0.5, 1.5, E).astype(f32), ss=rng.uniform(0.5, 1.5, E).astype(f32),
               sd=rng.uniform(0.5, 1.5, n).astype(f32), self_=nrm(n, D), prev=nrm(n, D), add=nrm(n, D))
    return s, t, ops


def hop_ref(D, transposed, combo, seed=0, dtype=f64):
    s, t, ops = hop_case(D, transposed, seed)
    kw = {k: ops[k].astype(dtype) for k, on in zip(FIELDS, combo) if on}
    return hop(s, t, N_NODES, ops["z"].astype(dtype), alpha=ALPHA, beta=BETA if "self_" in kw else 0.0, gam=GAMMA if "prev" in kw else 0.0, **kw)


def hop_condition(D, transposed, seed=0):
    """the worst norm-wise distance of the float32 restatement from float64 over the 64 combinations"""
    return max(rel(hop_ref(D, transposed, c, seed, f32), hop_ref(D, transposed, c, seed, f64)) for c in COMBOS)


# ---- ChebConv --------------------------------------------------------------------------------------------------------------------------
def cheb_c(s, n, w, dtype):
    """1 / sqrt(out-degree), weighted when the graph has weights"""
    d = np.bincount(s, weights=None if w is None else w.astype(f64), minlength=n).astype(dtype)
    return (1 / np.sqrt(d)).astype(dtype)


def cheb_forward(s, t, n, x, W, b, lam, w=None, keep=None):
    """Y [n][out]; W [k][out][in]; lam: λmax, an argument (the GPU tests pass the value the device path used)"""
    c = cheb_c(s, n, w, x.dtype)
    a, bb = 2.0 / lam, 2.0 / lam - 1.0
    Z = [x]
    if len(W) > 1:
        Z.append(hop(s, t, n, x, w, c[s], c, -a, bb, x))
    for _ in range(2, len(W)):
        Z.append(hop(s, t, n, Z[-1], w, c[s], c, -2 * a, 2 * bb, Z[-1], -1.0, Z[-2]))
    Y = sum(Zk @ Wk.T for Zk, Wk in zip(Z, W))
    if keep is not None:
        keep["Z"] = Z
    return Y if b is None else Y + b


def cheb_grad(s, t, n, x, W, b, lam, dY, w=None):
    """dict(Y, dx, dW, db, mag_W, mag_b) for the loss Σ Y ⊙ dY: dW_k = ΔY' Z_k; Δx by Clenshaw over the TRANSPOSED operator —
    B_K = G_K, B_k = G_k + 2 L̃ᵀ B_{k+1} - B_{k+2}, Δx = G_1 + L̃ᵀ B_2 - B_3 with G_k = ΔY W_k"""
    k = {}
    Y = cheb_forward(s, t, n, x, W, b, lam, w, k)
    Z, K = k["Z"], len(W)
    c = cheb_c(s, n, w, x.dtype)
    a, bb = 2.0 / lam, 2.0 / lam - 1.0
    B1 = B2 = None
    for q in range(K, 0, -1):
        G = dY @ W[q - 1]
        if B1 is None:
            B = G
        else:
            two = 2.0 if q >= 2 else 1.0
            B = hop(t, s, n, B1, w, c[t], c, -two * a, two * bb, B1, -1.0 if B2 is not None else 0.0, B2, G)
        B1, B2 = B, B1
    dW = np.stack([dY.T @ Zk for Zk in Z])
    mag = np.stack([np.abs(dY).T @ np.abs(Zk) for Zk in Z])
    return dict(Y=Y, dx=B1, dW=dW, db=dY.sum(0), mag_W=mag, mag_b=np.abs(dY).sum(0))


# ---- DConv -----------------------------------------------------------------------------------------------------------------------------
def dconv_slices(k):
    """the weight slice of each term T_0 .. T_k of a direction, as the reference wrote the loop (slice 1, 0-based, twice)"""
    return [0] if k == 1 else [0, 1] + list(range(1, k))


def _dconv_dirs(s, t, n, w, dtype):
    """per direction d (0 feeds weights[0]: steps over gᵀ with the in-degree; 1 feeds weights[1]: steps over g with the out-degree):
    (step, its adjoint)"""
    ww = None if w is None else w.astype(f64)
    deg_out, deg_in = np.bincount(s, weights=ww, minlength=n).astype(dtype), np.bincount(t, weights=ww, minlength=n).astype(dtype)
    S_out = lambda T_, **kw: hop(s, t, n, T_, w, deg_out[s], **kw)            # noqa: E731
    S_in = lambda T_, **kw: hop(t, s, n, T_, w, deg_in[t], **kw)              # noqa: E731
    S_out_T = lambda D_: hop(t, s, n, D_, w, None, deg_out)                   # noqa: E731
    S_in_T = lambda D_: hop(s, t, n, D_, w, None, deg_in)                     # noqa: E731
    return ((S_in, S_in_T), (S_out, S_out_T))


def dconv_forward(s, t, n, x, W, b, w=None, keep=None):
    """h [n][out]; W [2][k][out][in]"""
    k = W.shape[1]
    idx = dconv_slices(k)
    dirs = _dconv_dirs(s, t, n, w, x.dtype)
    T = [[x], [x]]
    for d in (0, 1):
        S = dirs[d][0]
        if k > 1:
            T[d].append(S(x))
        for _ in range(1, k):
            T[d].append(S(T[d][-1], alpha=2.0, gam=-1.0, prev=x))
    h = sum(T[0][j] @ W[0, i].T + T[1][j] @ W[1, i].T for j, i in enumerate(idx))
    if keep is not None:
        keep["T"] = T
    return h if b is None else h + b


def dconv_grad(s, t, n, x, W, b, dY, w=None):
    """dict(Y, dx, dW, db, mag_W, mag_b): reverse accumulation over the forward as written — dT_j += ΔY W[d, slice_j]; for j = k .. 2:
    dT_{j-1} += 2 Sᵀ dT_j and Δx -= dT_j; Δx += Sᵀ dT_1 + dT_0"""
    keep = {}
    Y = dconv_forward(s, t, n, x, W, b, w, keep)
    T = keep["T"]
    k = W.shape[1]
    idx = dconv_slices(k)
    dirs = _dconv_dirs(s, t, n, w, x.dtype)
    dW, mag, dx = np.zeros_like(W), np.zeros_like(W), np.zeros_like(x)
    for d in (0, 1):
        ST = dirs[d][1]
        dT = [dY @ W[d, i] for i in idx]
        for j, i in enumerate(idx):
            dW[d, i] += dY.T @ T[d][j]
            mag[d, i] += np.abs(dY).T @ np.abs(T[d][j])
        for j in range(len(idx) - 1, 1, -1):
            dT[j - 1] = dT[j - 1] + 2 * ST(dT[j])
            dx = dx - dT[j]
        if len(idx) > 1:
            dx = dx + ST(dT[1])
        dx = dx + dT[0]
    return dict(Y=Y, dx=dx, dW=dW, db=dY.sum(0), mag_W=mag, mag_b=np.abs(dY).sum(0))


# ---- the layer cases -------------------------------------------------------------------------------------------------------------------
def bidirected_graph(n=30, extra=40, seed=3):
    """(s, t) 0-based, every undirected pair once in each direction, no self loops, no repeated edge, no isolated node (a ring + extras)"""
    rng = np.random.default_rng([seed, 21])
    pairs = {(i, (i + 1) % n) if i < (i + 1) % n else ((i + 1) % n, i) for i in range(n)}
    while len(pairs) < n + extra:
        i, j = sorted(rng.integers(0, n, 2))
        if i != j:
            pairs.add((int(i), int(j)))
    pairs = np.array(sorted(pairs))
    perm = rng.permutation(2 * len(pairs))
    s, t = np.concatenate([pairs[:, 0], pairs[:, 1]])[perm], np.concatenate([pairs[:, 1], pairs[:, 0]])[perm]
    return s.astype(np.int64), t.astype(np.int64), n


def directed_graph(n=24, E=60, seed=4):
    """(s, t) 0-based, directed, with a repeated edge and a self loop; in- and out-degrees stay small (DConv multiplies by them)"""
    rng = np.random.default_rng([seed, 22])
    s, t = rng.integers(0, n, E), rng.integers(0, n, E)
    s[1], t[1] = s[0], t[0]
    s[2] = t[2]
    return s.astype(np.int64), t.astype(np.int64), n


CHEB_KS, CHEB_WEIGHTS, CHEB_SHAPE = (1, 2, 3, 5), ("none", "symmetric", "asymmetric"), (12, 10)
DCONV_KS, DCONV_SHAPE = (1, 2, 3), (9, 7)
CHEB_CASES = [(k, bias, wk) for k in CHEB_KS for bias in (True, False) for wk in CHEB_WEIGHTS]
DCONV_CASES = [(k, weighted) for k in DCONV_KS for weighted in (False, True)]


def cheb_weights(kind, seed=0):
    s, t, n = bidirected_graph()
    if kind == "none":
        return None
    rng = np.random.default_rng([seed, 23])
    w = rng.uniform(0.5, 1.5, len(s)).astype(f32)
    if kind == "symmetric":
        tab = {}
        for q in range(len(s)):
            key = (min(s[q], t[q]), max(s[q], t[q]))
            w[q] = tab.setdefault(key, w[q])
    return w


def cheb_case(k, bias, kind, seed=0):
    """(x, W, b, w, dY) float32 on bidirected_graph()"""
    s, t, n = bidirected_graph()
    nin, out = CHEB_SHAPE
    rng = np.random.default_rng([seed, k, int(bias), CHEB_WEIGHTS.index(kind), 24])
    x = rng.standard_normal((n, nin)).astype(f32)
    W = np.stack([glorot(rng, out, nin) for _ in range(k)])
    b = (0.1 * rng.standard_normal(out)).astype(f32) if bias else None
    return x, W, b, cheb_weights(kind), rng.standard_normal((n, out)).astype(f32)


def cheb_lam(kind):
    """λmax as the reference takes it: eigmax of Symmetric(L), the upper triangle of L = I - Ã (dense, float64)"""
    s, t, n = bidirected_graph()
    w = cheb_weights(kind)
    A = np.zeros((n, n))
    np.add.at(A, (s, t), 1.0 if w is None else w.astype(f64))
    c = 1 / np.sqrt(A.sum(1))
    Lm = np.eye(n) - c[:, None] * A * c[None, :]
    return float(np.linalg.eigvalsh(np.triu(Lm) + np.triu(Lm, 1).T)[-1])


def _c(v, dtype):
    return None if v is None else v.astype(dtype)


_REF = {}


def cheb_ref(k, bias, kind, lam, dtype=f64):
    """cheb_grad for cheb_case in `dtype`; the float64 result is computed once per (case, lam) and shared"""
    key = ("cheb", k, bias, kind, lam, dtype)
    if key not in _REF:
        s, t, n = bidirected_graph()
        x, W, b, w, dY = cheb_case(k, bias, kind)
        _REF[key] = cheb_grad(s, t, n, x.astype(dtype), W.astype(dtype), _c(b, dtype), lam, dY.astype(dtype), _c(w, dtype))
    return _REF[key]


def cheb_condition(k, bias, kind, lam):
    got, ref = cheb_ref(k, bias, kind, lam, f32), cheb_ref(k, bias, kind, lam, f64)
    return max(rel(got[q], ref[q]) for q in ("Y", "dx", "dW", "db"))


def dconv_case(k, weighted, seed=0):
    """(x, W, b, w, dY) float32 on directed_graph()"""
    s, t, n = directed_graph()
    nin, out = DCONV_SHAPE
    rng = np.random.default_rng([seed, k, int(weighted), 25])
    x = rng.standard_normal((n, nin)).astype(f32)
    W = np.stack([np.stack([glorot(rng, out, nin) for _ in range(k)]) for _ in range(2)])
    b = (0.1 * rng.standard_normal(out)).astype(f32)
    w = rng.uniform(0.5, 1.5, len(s)).astype(f32) if weighted else None
    return x, W, b, w, rng.standard_normal((n, out)).astype(f32)


def dconv_ref(k, weighted, dtype=f64):
    key = ("dconv", k, weighted, dtype)
    if key not in _REF:
        s, t, n = directed_graph()
        x, W, b, w, dY = dconv_case(k, weighted)
        _REF[key] = dconv_grad(s, t, n, x.astype(dtype), W.astype(dtype), _c(b, dtype), dY.astype(dtype), _c(w, dtype))
    return _REF[key]


def dconv_condition(k, weighted):
    got, ref = dconv_ref(k, weighted, f32), dconv_ref(k, weighted, f64)
    return max(rel(got[q], ref[q]) for q in ("Y", "dx", "dW", "db"))


def sum_n(n_nodes, n_edges, orders):
    """THE n OF THE WEIGHT GRADIENTS' BOUND γ_n Σ|terms|.  dW_k = ΔY' Z_k is a sum over the N node rows, but its terms are not exact
    inputs: Z_k is the k-th link of a chain of hops, each a fold of at most E slots plus three epilogue terms.  To first order the
    roundings of a chain of sums add, so n = N + orders * (E + 3): the sum's own length plus every addition on the longest path from
    an input to one of its terms (the convention of tests/megnet_conv_ref.py: the longest fold on the path, here once per order)."""
    return n_nodes + orders * (n_edges + 3)
