"""numpy restatements of ppr_diffusion (GNNGraphs/src/transform.jl:1026-1051) for tests/test_ppr_ref.py, tests/test_ppr.py, tests/test_ppr_abi.py
and the case table of tests/abi_cases.py:

  matrix32   the reference's Float32 matrix: A[t, s] accumulated in edge order, M = I + (alpha32 - 1) * A (product rounded, then added)
  ref64      (a) the reference in float64, FORMED FROM the float32-rounded M: alpha32 * inv(float64(M32)) read at the edges.  The input
             rounding is the reference's own, so what is left between it and a float32 result is the float32 inversion alone.
  lapack32   (b) the same with np.linalg.inv on the float32 matrix — LAPACK's sgetrf / sgetri, which is what the reference's `inv` calls.
  restate32  (c) csrc/ppr.hip's elimination in numpy float32: in-place Gauss-Jordan, the pivot the largest |a_ik| over the rows i >= k with
             the lowest row on a tie, an exactly zero pivot reported, the pivot row r_j = (j == k ? 1 : a_kj) / piv, every other row
             a_ij = fma(-f_i, r_j, j == k ? 0 : a_ij) with the fused multiply-add emulated through float64 (the product of two float32
             is exact in float64; the sum is rounded to float64, then to float32), the exchanges undone on the columns last first.

Graphs are (s, t, n, w): 0-based int64 numpy arrays, w float32 or None.  Results are float arrays [n_edges] in edge order.

THE BAR of the device tests, element-wise against ref64:
    |got - ref64| <= K * max(max|lapack32 - ref64|, 2^-24 * max|ref64|)
K comes from restate32 and the reference alone, never from a device: for every input of tests/test_ppr.py the ratio
max|restate32 - ref64| / max(max|lapack32 - ref64|, 2^-24 max|ref64|) was computed on the CPU (tests/test_ppr_ref.py recomputes it and
checks that none exceeds K / 2), and K is twice the worst, rounded up.  The table (numpy 2.x, OpenBLAS LAPACK):

    input        nodes  edges  cond(M)  ratio        input        nodes  edges  cond(M)  ratio
    n1_u             1      1    1.000  1.000        n1_w             1      1    1.000  0.297
    n2_u             2      6    2.343  0.724        n2_w             2      6    1.348  0.917
    n5_u             5     15    3.219  1.000        n5_w             5     15    1.783  1.506
    n12_u           12     36    3.023  1.000        n12_w           12     36    1.754  0.888
    n33_u           33     99    3.028  1.595        n33_w           33     99    1.754  1.934
    n64_u           64    192    2.772  2.649        n64_w           64    192    1.738  1.509
    n65_u           65    195    2.825  2.804        n65_w           65    195    1.801  3.354
    n127_u         127    381    2.954  3.974        n127_w         127    381    1.711  1.541
    batch_u        309    925    4.474  1.370        batch_w        309    925    2.044  2.300
    large300_w     300   1200    2.015  7.457        pivot            2      3    5.828  0.000
    two_cycle        2      2    3.000  0.500        alpha1           3      6    1.000  0.000
    n150_w         150    450    1.758  1.476        exchange70      70    210    2.356  1.746
  worst 7.457 (large300_w, where the floor 2^-24 max|ref64| governs: LAPACK's own error there is 3.1e-8)  ->  K = ceil(2 * 7.457) = 15
"""
import functools

import numpy as np

f32, f64 = np.float32, np.float64
ALPHA = 0.85
COND_BAR = 10.0         # every device input: cond_2(M) < 10 in float64 (a condition on the inputs, tests/test_ppr_ref.py)
K = 15                  # twice the worst ratio of the table above, rounded up
SIZES = (1, 2, 5, 12, 33, 64, 65, 127)
LARGE = 300
OPT_IN = 150
EXCHANGE = 70


class Singular(Exception):
    """restate32 met an exactly zero pivot at elimination step .step"""

    def __init__(self, step):
        super().__init__(f"zero pivot at step {step}")
        self.step = step


def matrix32(s, t, n, w, alpha):
    a32 = f32(alpha)
    w = np.ones(len(s), f32) if w is None else np.asarray(w, f32)
    A = np.zeros((n, n), f32)
    for e in range(len(s)):                                      # edge order; float32 adds
        A[t[e], s[e]] = f32(A[t[e], s[e]] + w[e])
    return (np.eye(n, dtype=f32) + (f32(a32 - f32(1.0)) * A).astype(f32)).astype(f32)


def ref64(s, t, n, w, alpha):
    if n == 0 or len(s) == 0:
        return np.zeros(0, f64)
    P = f64(f32(alpha)) * np.linalg.inv(matrix32(s, t, n, w, alpha).astype(f64))
    return P[t, s]


def lapack32(s, t, n, w, alpha):
    if n == 0 or len(s) == 0:
        return np.zeros(0, f32)
    M = matrix32(s, t, n, w, alpha)
    inv = np.linalg.inv(M)
    assert inv.dtype == f32
    return (f32(alpha) * inv).astype(f32)[t, s]


def fma32(x, y, z):
    """fma(x, y, z) on float32 arrays through float64"""
    return (x.astype(f64) * y.astype(f64) + z.astype(f64)).astype(f32)


def inverse32(M, exchanges=None):
    """the in-place elimination of csrc/ppr.hip on a float32 matrix; raises Singular.  exchanges: a list that receives (k, p) of every
    step whose pivot row p is not k"""
    a = np.array(M, f32)
    n = a.shape[0]
    perm = np.arange(n)
    for k in range(n):
        f = a[:, k].copy()
        mag = np.abs(f[k:])
        p = k
        if not np.all(np.isnan(mag)):
            p = k + int(np.flatnonzero(mag == np.nanmax(mag))[0])   # the lowest row among the largest
        piv = f[p]
        if piv == 0:
            raise Singular(k)
        perm[k] = p
        if p != k:
            if exchanges is not None:
                exchanges.append((k, p))
            a[[k, p]] = a[[p, k]]
            f[p] = f[k]                                          # the row that came from k: its f is the old a_kk
        row = a[k].copy()
        row[k] = f32(1.0)
        with np.errstate(all="ignore"):
            r = (row / piv).astype(f32)
        a[k] = r
        addend = a.copy()
        addend[:, k] = 0
        with np.errstate(all="ignore"):
            upd = fma32(-f[:, None], r[None, :], addend)
        upd[k] = r
        a = upd
    src = np.arange(n)
    for k in range(n - 1, -1, -1):
        p = perm[k]
        if p != k:
            src[k], src[p] = src[p], src[k]
    return a[:, src]


def restate32(s, t, n, w, alpha):
    if n == 0 or len(s) == 0:
        return np.zeros(0, f32)
    inv = inverse32(matrix32(s, t, n, w, alpha))
    return (f32(alpha) * inv).astype(f32)[t, s]


def bar_scale(lap, r64):
    """max(max|lapack32 - ref64|, 2^-24 * max|ref64|): the reference's own float32 error on this input, floored at half an ulp of the
    largest result"""
    if len(r64) == 0:
        return 0.0
    return max(float(np.abs(lap.astype(f64) - r64).max()), 2.0 ** -24 * float(np.abs(r64).max()))


def ratio(got, lap, r64):
    """max|got - ref64| in units of bar_scale"""
    if len(r64) == 0:
        return 0.0
    return float(np.abs(np.asarray(got, f64) - r64).max()) / bar_scale(lap, r64)


def within_bar(got, lap, r64):
    got = np.asarray(got)
    return got.shape == r64.shape and bool(np.all(np.isfinite(got))) and ratio(got, lap, r64) <= K


def cond(s, t, n, w, alpha):
    return float(np.linalg.cond(matrix32(s, t, n, w, alpha).astype(f64))) if n else 1.0


# ---- the graphs --------------------------------------------------------------------------------------------------------------------
def _g(s, t, n, w=None):
    return (np.asarray(s, np.int64).reshape(-1), np.asarray(t, np.int64).reshape(-1), int(n), None if w is None else np.asarray(w, f32))


def random_graph(n, seed, weights=False, per_node=3):
    """a random multigraph: about per_node in-edges a node (mean in-degree <= 4), weights in [0.1, 1] or none.  From 5 nodes on the last
    node is isolated, edge 1 repeats edge 0 (a multi-edge) and edge 2 is a self loop"""
    rng = np.random.default_rng(seed)
    E = n * per_node if n > 1 else 1
    hi = n - 1 if n >= 5 else n
    s, t = rng.integers(0, hi, E), rng.integers(0, hi, E)
    if n >= 5:
        s[1], t[1] = s[0], t[0]
        t[2] = s[2]
    return _g(s, t, n, rng.uniform(0.1, 1.0, E) if weights else None)


PIVOT = (_g([0, 0, 1], [0, 1, 0], 2, [2.0, 1.0, 1.0]), 0.5)          # M = [0 -0.5; -0.5 1]: M[1, 1] = 0 exactly, a swap is needed
PIVOT_ANSWER = np.array([-2.0, -1.0, -1.0], f32)                     # 0.5 * inv(M) = [-2 -1; -1 0]
SINGULAR = (_g([0], [0], 1, [2.0]), 0.5)                             # M = [0]
TWO_CYCLE = (_g([0, 1], [1, 0], 2), 0.5)                             # 0.5 * inv([1 -0.5; -0.5 1]) = [2/3 1/3; 1/3 2/3]


def members(weights):
    return [random_graph(n, (500 if weights else 400) + i, weights) for i, n in enumerate(SIZES)]


def concat(graphs, empties=()):
    """the block-diagonal graph, member by member (edges too), and its node offsets; empties: positions (in the final list of members) at
    which a member without nodes is inserted"""
    off = [0]
    for m in graphs:
        off.append(off[-1] + m[2])
    s = np.concatenate([m[0] + o for m, o in zip(graphs, off)])
    t = np.concatenate([m[1] + o for m, o in zip(graphs, off)])
    ws = [m[3] for m in graphs]
    w = None if any(x is None for x in ws) else np.concatenate(ws)
    for pos in sorted(empties):
        off.insert(pos, off[pos])
    return _g(s, t, off[-1], w), np.asarray(off, np.int64)


BATCH_EMPTIES = (3, 9)      # after the third member, and at the end: 10 members, two of them empty


def batch(weights):
    """-> (graph, node offsets [11], edge offsets of the 8 real members [9])"""
    ms = members(weights)
    g, off = concat(ms, BATCH_EMPTIES)
    eoff = np.concatenate([[0], np.cumsum([len(m[0]) for m in ms])])
    return g, off, eoff


def large_graph():
    return random_graph(LARGE, 300, weights=True, per_node=4)


def opt_in_graph():
    """150 nodes: above the default LDS budget of csrc/ppr.hip (127 nodes), inside the largest (201 nodes)"""
    return random_graph(OPT_IN, 150, weights=True)


def exchange_graph():
    """70 nodes (a pivot column spans two waves) whose elimination exchanges rows at almost every step, alpha = 0.5: one edge of weight
    5 .. 7 from every node to its image under a random permutation, so column k of M = I - 0.5 A holds 1 on the diagonal and about -3
    in row perm(k), plus 140 light edges (0.1 .. 0.3); shuffled.  I - 3 P is normal with eigenvalues of modulus 2 .. 4: well conditioned"""
    n, rng = EXCHANGE, np.random.default_rng(700)
    s2, t2 = rng.integers(0, n, 2 * n), rng.integers(0, n, 2 * n)
    s = np.concatenate([np.arange(n), s2])
    t = np.concatenate([rng.permutation(n), t2])
    w = np.concatenate([rng.uniform(5.0, 7.0, n), rng.uniform(0.1, 0.3, 2 * n)])
    order = rng.permutation(3 * n)
    return _g(s[order], t[order], n, w[order])


def random_cases():
    """name -> (graph, alpha) of every random input of tests/test_ppr.py"""
    out = {}
    for wt in (False, True):
        tag = "w" if wt else "u"
        for m in members(wt):
            out[f"n{m[2]}_{tag}"] = (m, ALPHA)
        out[f"batch_{tag}"] = (batch(wt)[0], ALPHA)
    out["n150_w"] = (opt_in_graph(), ALPHA)
    out["large300_w"] = (large_graph(), ALPHA)
    return out


def known_cases():
    return {"pivot": PIVOT, "two_cycle": TWO_CYCLE, "exchange70": (exchange_graph(), 0.5),
            "alpha1": (_g([0, 0, 1, 2, 2, 1], [0, 1, 2, 2, 0, 1], 3, [0.5, 1.0, 0.25, 2.0, 1.0, 0.75]), 1.0)}


@functools.lru_cache(maxsize=None)
def references():
    """name -> (graph, alpha, ref64, lapack32) for every device input, computed once per process"""
    return {name: (g, al, ref64(*g, al), lapack32(*g, al)) for name, (g, al) in {**random_cases(), **known_cases()}.items()}
