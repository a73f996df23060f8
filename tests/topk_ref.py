"""numpy restatement of TopKPool / topk_index (GNNlib/src/layers/pool.jl:14-27) and of the order include/gnnmp.h states for
gnnmp_topk_select_f32.  The selection here SORTS (a stable argsort on the descending key); the device counts — two statements of one
order.  Everything is host arithmetic: float64 for values, integers for the selection.

    y   = p' * X / norm(p)
    idx = topk_index(y, k)          # collect(1:n)[y .>= nlargest(k, y)[end]], ascending
    A~  = view(A, idx, idx)
    X_  = view(X, :, idx) .* σ.(view(y, idx)')
"""
import math

import numpy as np

FIRST, ALL = 0, 1
SIGMOID, TANH, IDENTITY = 0, 1, 2
ACTS = {"sigmoid": SIGMOID, "tanh": TANH, "identity": IDENTITY}
GRAD_ROWS = 64      # include/gnnmp.h: GNNMP_TOPK_GRAD_ROWS


def keys(y):
    """the uint32 key of every fp32 score: the monotone map of the bits after -0.0 became +0.0; every NaN is key 0 (below -Inf)"""
    b = np.ascontiguousarray(y, np.float32).reshape(-1).view(np.uint32).copy()
    nan = (b & np.uint32(0x7fffffff)) > np.uint32(0x7f800000)
    b[b == np.uint32(0x80000000)] = 0
    neg = (b & np.uint32(0x80000000)) != 0
    k = np.where(neg, ~b, b | np.uint32(0x80000000)).astype(np.uint32)
    k[nan] = 0
    return k


def ranks(key):
    """0-based rank of every position: larger keys first, equal keys by ascending position (a stable sort of the descending key)"""
    order = np.argsort(-key.astype(np.int64), kind="stable")
    r = np.empty(len(key), np.int64)
    r[order] = np.arange(len(key))
    return r


def k_of(n, k, ratio):
    """k_g of a member graph of n nodes: min(n, k), or with k == 0 min(n, ceil((double) ratio * (double) n)) — ratio is the record's
    float, widened: (float) 0.1 * 30 = 3.0000000447 in double, and the ceiling is 4"""
    return min(n, int(k)) if k > 0 else min(n, int(math.ceil(float(np.float32(ratio)) * float(n))))


def select(y, ptr=None, k=0, ratio=0.0, ties=FIRST):
    """(keep uint32 [N + 1] with keep[N] = 0, rank int32 [N]) per member graph [ptr[g], ptr[g + 1]) — ptr None: one graph"""
    y = np.asarray(y, np.float32).reshape(-1)
    N = len(y)
    ptr = np.array([0, N]) if ptr is None else np.asarray(ptr, np.int64)
    key = keys(y)
    keep, rank = np.zeros(N + 1, np.uint32), np.zeros(N, np.int32)
    for a, b in zip(ptr[:-1], ptr[1:]):
        n = int(b - a)
        if n == 0:
            continue
        kk = key[a:b]
        r = ranks(kk)
        kg = k_of(n, k, ratio)
        rank[a:b] = r
        if ties == FIRST:
            keep[a:b] = r < kg
        else:
            keep[a:b] = kk >= kk[r == kg - 1][0]
    return keep, rank


def topk_index_julia(y, k):
    """the reference's two lines, literally (1-based): v = nlargest(k, y); collect(1:length(y))[y .>= v[end]]"""
    y = np.asarray(y).reshape(-1)      # (topk_index(y::Adjoint, k) = topk_index(y', k): the row form is the vector)
    v = np.sort(y)[::-1][:k]
    return np.flatnonzero(y >= v[-1]) + 1


def topk_index(y, k, ties=ALL):
    """1-based ascending positions through `select` (one graph)"""
    keep, _ = select(y, None, k, 0.0, ties)
    return np.flatnonzero(keep[:-1]) + 1


def act64(code, y):
    y = np.asarray(y, np.float64)
    if code == SIGMOID:
        return 1.0 / (1.0 + np.exp(-y))
    if code == TANH:
        return np.tanh(y)
    return y


def score64(x, p):
    x, p = np.asarray(x, np.float64), np.asarray(p, np.float64)
    return x @ p / np.sqrt((p * p).sum())


def gate64(x, y, idx0, act):
    """x2 [len(idx0)][C] = x[idx0] * act(y[idx0]) in float64"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    return x[idx0] * act64(act, y[idx0])[:, None]


def induced(s0, t0, keep):
    """(s2, t2, eid) of the subgraph on the kept nodes: 0-based, nodes renumbered in ascending order, edges in their order"""
    keep = np.asarray(keep).astype(bool)      # [N]: without the closing word
    new = np.cumsum(keep) - 1
    m = keep[s0] & keep[t0]
    return new[s0[m]], new[t0[m]], np.flatnonzero(m)


def topk_pool(x, p, s0, t0, ptr=None, k=0, ratio=0.0, act=SIGMOID, y32=None):
    """the batched layer: (idx0, x2 float64, s2, t2, eid).  The selection is taken on y32 (fp32 scores: the device's own, read back) —
    by default the float32 rounding of the float64 score, which the caller must know to be exact"""
    y = score64(x, p)
    ysel = np.asarray(y, np.float32) if y32 is None else np.asarray(y32, np.float32)
    keep, _ = select(ysel, ptr, k, ratio, FIRST)
    kept = keep[:-1].astype(bool)
    idx0 = np.flatnonzero(kept)
    s2, t2, eid = induced(np.asarray(s0), np.asarray(t0), kept)
    return idx0, gate64(x, y, idx0, act), s2, t2, eid


def topk_pool_julia(A, X, p, k):
    """the reference's layer on its own layout: A [N][N], X [C][N] -> (X_ [C][k], A~ [k][k])"""
    X, p = np.asarray(X, np.float64), np.asarray(p, np.float64)
    y = p @ X / np.sqrt((p * p).sum())
    idx = topk_index_julia(y, k) - 1
    return X[:, idx] * act64(SIGMOID, y[idx])[None, :], np.asarray(A)[np.ix_(idx, idx)]


# ---- the score vectors and the batch of tests/test_topk_pool.py and tests/topk_cases.py -----------------------------------------------
SIZES = (0, 1, 2, 63, 64, 65, 255, 256, 257, 1030)


def batch_ptr(sizes=SIZES):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def score_vectors(ptr, k_hint=4, seed=0):
    """{name: float32 [N]} over the batch `ptr`: random, all equal, a tie block straddling rank k_hint in every member graph, negative
    only, specials (±0, ±Inf, denormals, NaNs of both signs), strictly descending and ascending"""
    rng = np.random.default_rng(seed)
    N = int(ptr[-1])
    out = {"random": rng.standard_normal(N).astype(np.float32), "equal": np.full(N, 0.25, np.float32)}
    tie = np.empty(N, np.float32)
    for a, b in zip(ptr[:-1], ptr[1:]):
        n = int(b - a)
        v = -np.arange(n, dtype=np.float32)                    # descending ...
        lo, hi = max(0, k_hint - 2), min(n, k_hint + 3)
        v[lo:hi] = -float(lo)                                   # ... with equal values on ranks k - 2 .. k + 2
        tie[a:b] = v[rng.permutation(n)]
    out["tie_block"] = tie
    out["negative"] = (-1.0 - rng.random(N)).astype(np.float32)
    pool = np.array([0.0, -0.0, np.inf, -np.inf, 1e-45, -1e-45, 1e-39, -1e-39, 1.0, -1.0], np.float32)
    sp = pool[rng.integers(0, len(pool), N)].copy()
    nan = rng.random(N) < 0.2
    bits = sp.view(np.uint32)
    bits[nan] = np.where(rng.random(int(nan.sum())) < 0.5, np.uint32(0x7fc00001), np.uint32(0xffc12345))      # NaNs, both signs
    out["specials"] = sp
    out["descending"] = (-np.arange(N, dtype=np.float32))
    out["ascending"] = np.arange(N, dtype=np.float32)
    return out
