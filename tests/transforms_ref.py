"""numpy restatement of the reference's edge-list transforms, line by line, for tests/test_transforms_abi.py (which checks it against the
reference's own test items) and tests/test_transforms.py (which checks the device against it):

  remove_self_loops / remove_edges / remove_multi_edges     GNNGraphs/src/transform.jl:49-185
  to_bidirected / to_unidirected                            GNNGraphs/src/transform.jl:495-529
  edge_encoding / edge_decoding                             GNNGraphs/src/utils.jl:189-260
  has_isolated_nodes / has_multi_edges                      GNNGraphs/src/query.jl:420-422, 575-579

Indices are 1-based int64 like the reference's; edge data is laid out [E, ...] (Julia's (..., E)) and is float32: `_scatter` is NNlib's CPU
loop, a sequential fold in the order of the (stably sorted) edges, one float32 operation at a time."""
import numpy as np

f32 = np.float32


def edge_encoding(s, t, n, directed=True):
    s, t, n = np.asarray(s, np.int64), np.asarray(t, np.int64), int(n)
    if directed:
        return (s - 1) * n + t, n * n
    mask = s > t
    snew, tnew = s.copy(), t.copy()
    snew[mask], tnew[mask] = t[mask], s[mask]
    s, t = snew, tnew
    return (s - 1) * (2 * (n + 1) - s) // 2 + (t - s + 1), n * (n + 1) // 2


def edge_decoding(idx, n, directed=True):
    idx, n = np.asarray(idx, np.int64), int(n)
    if directed:
        return (idx - 1) // n + 1, (idx - 1) % n + 1
    # s = @. ceil(Int, -sqrt((n + 1 / 2)^2 - 2 * idx) + n + 1 / 2)  — Float64, exact for the node counts the tests use
    s = np.ceil(-np.sqrt((n + 0.5) ** 2 - 2.0 * idx.astype(np.float64)) + n + 0.5).astype(np.int64)
    t = idx - (s - 1) * (2 * (n + 1) - s) // 2 - 1 + s
    return s, t


def _map(data, f):
    if data is None:
        return None
    if isinstance(data, dict):
        return {k: _map(v, f) for k, v in data.items()}
    return f(np.asarray(data))


def getobs(data, sel):
    return _map(data, lambda a: a[sel])


def cat_features(a, b):
    if a is None:
        return None
    if isinstance(a, dict):
        return {k: cat_features(a[k], b[k]) for k in a}
    return np.concatenate([np.asarray(a), np.asarray(b)])


def scatter(aggr, src, idx, n):
    """NNlib.scatter(aggr, src, idx; dstsize = (..., n)) for an ASCENDING 1-based idx (what remove_multi_edges passes): dst starts at the
    operator's identity and takes src[k] for k = 1, 2, ... in turn, in float32; mean = scatter(+) ./ count."""
    def one(a):
        a = np.asarray(a, f32)
        idx0 = np.asarray(idx, np.int64) - 1
        assert np.all(np.diff(idx0) >= 0)
        cnt = np.bincount(idx0, minlength=n)
        start = np.concatenate([[0], np.cumsum(cnt)])[:-1]
        init = {"+": 0.0, "mean": 0.0, "max": -np.inf, "min": np.inf}[aggr]
        op = {"+": np.add, "mean": np.add, "max": np.maximum, "min": np.minimum}[aggr]
        dst = np.full((n,) + a.shape[1:], init, f32)
        for j in range(int(cnt.max()) if n else 0):
            rows = np.flatnonzero(cnt > j)
            dst[rows] = op(dst[rows], a[start[rows] + j]).astype(f32)
        if aggr == "mean":
            c = cnt.astype(f32).reshape((n,) + (1,) * (a.ndim - 1))
            dst = (dst / c).astype(f32)
        return dst
    return _map(src, one)


class Coalesced:
    """the result of remove_multi_edges and, for the tests' masks, perm (0-based sorted order) and the length of every output segment"""

    def __init__(self, s, t, w, edata, perm, seg_len):
        self.s, self.t, self.w, self.edata, self.perm, self.seg_len = s, t, w, edata, perm, seg_len


def remove_multi_edges(s, t, n, w=None, edata=None, aggr="+"):
    s, t = np.asarray(s, np.int64), np.asarray(t, np.int64)
    num_edges = len(s)
    idxs, _ = edge_encoding(s, t, n)
    perm = np.argsort(idxs, kind="stable")                    # sortperm is stable
    idxs = idxs[perm]
    s, t = s[perm], t[perm]
    edata = getobs(edata, perm)
    w = getobs(w, perm)
    idxs = np.concatenate([[-1], idxs])
    mask = idxs[1:] > idxs[:-1]
    seg_len = np.ones(num_edges, np.int64)
    if not np.all(mask):
        s, t = s[mask], t[mask]
        idxs = np.arange(1, num_edges + 1) - np.cumsum(~mask)
        num_edges = len(s)
        seg_len = np.bincount(idxs - 1, minlength=num_edges)
        w = scatter(aggr, w, idxs, num_edges)
        edata = scatter(aggr, edata, idxs, num_edges)
    return Coalesced(s, t, w, edata, perm, seg_len)


def to_bidirected(s, t, n, w=None, edata=None):
    s, t = np.asarray(s, np.int64), np.asarray(t, np.int64)
    snew, tnew = np.concatenate([s, t]), np.concatenate([t, s])          # the real concatenation
    return remove_multi_edges(snew, tnew, n, cat_features(w, w), cat_features(edata, edata), aggr="mean")


def to_unidirected(s, t, n, w=None, edata=None):
    idxs, _ = edge_encoding(s, t, n, directed=False)
    snew, tnew = edge_decoding(idxs, n, directed=False)
    return remove_multi_edges(snew, tnew, n, w, edata, aggr="mean")


def remove_self_loops(s, t, w=None, edata=None):
    s, t = np.asarray(s, np.int64), np.asarray(t, np.int64)
    mask = s != t
    return s[mask], t[mask], getobs(w, mask), getobs(edata, mask), np.flatnonzero(mask)


def remove_edges(s, t, edges_to_remove, w=None, edata=None):
    """edges_to_remove: 1-based positions (repeats allowed)"""
    s, t = np.asarray(s, np.int64), np.asarray(t, np.int64)
    mask = np.ones(len(s), bool)
    mask[np.asarray(edges_to_remove, np.int64) - 1] = False
    return s[mask], t[mask], getobs(w, mask), getobs(edata, mask), np.flatnonzero(mask)


def has_multi_edges(s, t, n):
    idxs, _ = edge_encoding(s, t, n)
    return len(np.unique(idxs)) < len(idxs)


def has_isolated_nodes(s, t, n, dir="out"):
    v = np.asarray(s if dir == "out" else t, np.int64)
    return bool(np.any(np.bincount(v - 1, minlength=n) == 0))
