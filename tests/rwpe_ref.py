"""numpy restatement of random_walk_pe (GNNGraphs/src/transform.jl:975-990) for tests/test_rwpe_abi.py and tests/test_rwpe.py, in two forms:

  dense64   the reference's algorithm in float64: A, deg = row sums, dinv = 1 ./ deg with Inf -> 0, RW = A * Diagonal(dinv), the diagonals
            of RW^k.  Two variants for the tests of the directed case: `row_scaled=True` is Diagonal(dinv) * A, whose powers have the SAME
            diagonals (a closed walk leaves every node it enters: both products hold one dinv per node visited), and `in_degree=True`
            takes deg from the column sums — the mistake a directed graph does tell apart.
  fold32    what csrc/rwpe.hip computes: float32, every row folded over its out-edges in original edge order, the product
            (w_e * dinv[j]) * v[j] rounded before it is added.

Graphs are (s, t, n, w): 0-based int64 numpy arrays, w float32 or None.  Results are (n, walk_length), the library's layout.  The cases
of the GPU tests are built here, once, with both references; test_rwpe_abi.py checks on the CPU that every one of them is well
conditioned (fold32 within BAR of dense64), so that a GPU failure is the kernel's."""
import functools

import numpy as np

BAR = 1e-5
f32 = np.float32


def dense64(s, t, n, w, K, row_scaled=False, in_degree=False):
    A = np.zeros((n, n), np.float64)
    np.add.at(A, (s, t), np.ones(len(s)) if w is None else np.asarray(w, np.float64))
    deg = A.sum(axis=0 if in_degree else 1)
    with np.errstate(divide="ignore"):
        dinv = 1.0 / deg
    dinv[np.isinf(dinv)] = 0.0
    RW = dinv[:, None] * A if row_scaled else A * dinv[None, :]
    out = RW.copy()
    pe = np.zeros((n, K), np.float64)
    pe[:, 0] = np.diag(out)
    for k in range(1, K):
        out = out @ RW
        pe[:, k] = np.diag(out)
    return pe


def fold32(s, t, n, w, K):
    w = np.ones(len(s), f32) if w is None else np.asarray(w, f32)
    deg = np.zeros(n, f32)
    for e in range(len(s)):                                  # (edge order restricted to a row is the row's plan order)
        deg[s[e]] = f32(deg[s[e]] + w[e])
    with np.errstate(divide="ignore"):
        dinv = (f32(1.0) / deg).astype(f32)
    dinv[np.isinf(dinv)] = 0.0
    coef = (w * dinv[t]).astype(f32)
    V = np.eye(n, dtype=f32)
    pe = np.zeros((n, K), f32)
    for k in range(K):
        nxt = np.zeros((n, n), f32)
        for e in range(len(s)):
            nxt[s[e]] += coef[e] * V[t[e]]                   # float32 product, then float32 add
        pe[:, k] = np.diag(nxt)
        V = nxt
    return pe


def deviation(got, ref):
    """(norm-wise, worst element-wise) relative deviation from the float64 reference; inf where got is non-zero on a zero of the model"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    zero = ref == 0
    if np.any(got[zero] != 0) or not np.all(np.isfinite(got)):
        return np.inf, np.inf
    if zero.all():
        return 0.0, 0.0
    return float(np.linalg.norm(got - ref) / np.linalg.norm(ref)), float(np.max(np.abs(got - ref)[~zero] / np.abs(ref)[~zero]))


def within_bar(got, ref):
    nw, ew = deviation(got, ref)
    return nw <= BAR and ew <= BAR


# ---- the graphs --------------------------------------------------------------------------------------------------------------------
def _g(s, t, n, w=None):
    return (np.asarray(s, np.int64).reshape(-1), np.asarray(t, np.int64).reshape(-1), int(n), None if w is None else np.asarray(w, f32))


def random_graph(n, per_node, seed, weights=False):
    """about per_node out-edges a node (repeats and self loops as they fall), shuffled"""
    rng = np.random.default_rng(seed)
    E = n * per_node if n > 1 else 1
    s, t = rng.integers(0, n, E), rng.integers(0, n, E)
    return _g(s, t, n, rng.uniform(0.5, 1.5, E) if weights else None)


KNOWN = _g([0, 1, 1, 2], [1, 0, 2, 1], 3)                    # s = [1,2,2,3], t = [2,1,3,2] — GNNGraphs/test/transform.jl:431-440
KNOWN_ANSWER = np.array([[0.0, 0.5, 0.0], [0.0, 1.0, 0.0], [0.0, 0.5, 0.0]], f32)      # (n, 3): the transpose of the reference's matrix
# directed, in- and out-degrees differ: out (3, 1, 2, 1, 1), in (1, 1, 2, 2, 2)
DIRECTED = _g([0, 0, 0, 1, 2, 2, 3, 4], [1, 2, 3, 2, 0, 4, 4, 3], 5)


def semantic_cases():
    """name -> (graph, walk_length)"""
    return {
        "sink": (_g([0, 1, 2, 0], [1, 2, 0, 3], 4), 6),                          # node 3 has no out-edge: dinv = 0
        "self_loop": (_g([0, 0, 1, 2], [0, 1, 2, 0], 3), 5),                     # non-zero already at k = 1
        "doubled_edge": (_g([0, 0, 0, 1, 2], [1, 1, 2, 0, 0], 3), 6),            # 0 -> 1 counts twice against 0 -> 2
        "weights": (_g([0, 1, 1, 2, 2, 3], [1, 0, 2, 1, 3, 2], 4, [0.5, 1.5, 0.75, 1.25, 1.0, 0.625]), 6),
        "walk_length_1": (_g([0, 1, 1, 2, 2], [1, 0, 2, 1, 2], 3), 1),
        "one_node_loop": (_g([0], [0], 1), 4),
        "one_node_bare": (_g([], [], 1), 3),
        "directed": (DIRECTED, 6),
    }


BATCH_WALK = 6


def batch_members(T):
    """node counts 1, 2, T - 1, T, T + 1, 2 T + 1, 65; about 3 out-edges a node"""
    return [random_graph(n, 3, 100 + i) for i, n in enumerate((1, 2, T - 1, T, T + 1, 2 * T + 1, 65))]


def batch_weighted_members(T):
    return [random_graph(n, 3, 200 + i, weights=True) for i, n in enumerate((T + 1, 3, 2 * T + 1))]


def concat(members):
    """the block-diagonal graph, member by member (edges too), and its node offsets"""
    off = np.concatenate([[0], np.cumsum([m[2] for m in members])]).astype(np.int64)
    s = np.concatenate([m[0] + o for m, o in zip(members, off)])
    t = np.concatenate([m[1] + o for m, o in zip(members, off)])
    ws = [m[3] for m in members]
    w = None if any(x is None for x in ws) else np.concatenate(ws)
    return _g(s, t, off[-1], w), off


LARGE = (300, 4, 6)                                           # one unbatched graph: 300 nodes, 1 200 edges, walk_length 6


def large_graph():
    return random_graph(LARGE[0], LARGE[1], 300, weights=True)


def random_cases(T):
    """name -> (graph, walk_length) of every random case of tests/test_rwpe.py"""
    out = {f"member{i}": (m, BATCH_WALK) for i, m in enumerate(batch_members(T))}
    out["batch"] = (concat(batch_members(T))[0], BATCH_WALK)
    out["batch_weighted"] = (concat(batch_weighted_members(T))[0], BATCH_WALK)
    out["large"] = (large_graph(), LARGE[2])
    return out


@functools.lru_cache(maxsize=None)
def references(T):
    """name -> (graph, walk_length, dense64, fold32) for every case, computed once per process"""
    out = {}
    for name, (g, K) in {**semantic_cases(), **random_cases(T)}.items():
        out[name] = (g, K, dense64(*g, K), fold32(*g, K))
    return out
