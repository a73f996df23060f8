"""A numpy restatement of the reference's structural augmentations on plain (s, t, w, n) — remove_nodes, add_edges, add_nodes and
perturb_edges (GNNGraphs/src/transform.jl:212-276, 319-353, 385-420, 553-561) — with the two random draws restated from the library's
dropout hash (csrc/common.h: drop_mix32 / drop_bits / make_drop): the node mask of remove_nodes(g, p) and the pair draw of
perturb_edges.  Indices are in `base` (1 like the reference, or 0); the maps returned next to the graphs are 0-based."""
import math

import numpy as np

_M32 = 0xFFFFFFFF


def _mix32(x):
    x = np.asarray(x, np.uint64) & _M32
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7feb352d)) & _M32
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846ca68b)) & _M32
    x ^= x >> np.uint64(16)
    return x


def drop_bits(seed, e, h):
    """the 32 bits of (seed, e, h): drop_mix32(drop_mix32(e ^ seed_lo) ^ (h * 0x9e3779b9 + seed_hi))"""
    lo, hi = np.uint64(seed & _M32), np.uint64((seed >> 32) & _M32)
    e = np.asarray(e, np.uint64) & _M32
    h = np.asarray(h, np.uint64) & _M32
    return _mix32(_mix32(e ^ lo) ^ ((h * np.uint64(0x9e3779b9) + hi) & _M32))


def keep_mask(seed, p, n):
    """keep[i] of gnnmp_dropout_keep_u8(seed, p, n, 1), extended to p = 1 (nothing kept): bits >= floor(p 2^32), p as a Float32"""
    p = float(np.float32(p))
    if p >= 1.0:
        return np.zeros(n, bool)
    thr = min(int(p * 4294967296.0), _M32)
    return drop_bits(seed, np.arange(n), 0) >= np.uint64(thr)


def rand_pairs(seed, m, N):
    """pair k of gnnmp_plan_add_edges' random mode, 0-based: s = mulhi32(h(k, 0), N), t' = mulhi32(h(k, 1), N - 1), t = t' + (t' >= s)"""
    k = np.arange(m)
    s = (drop_bits(seed, k, 0) * np.uint64(N)) >> np.uint64(32)
    tp = (drop_bits(seed, k, 1) * np.uint64(N - 1)) >> np.uint64(32)
    t = tp + (tp >= s).astype(np.uint64)
    return s.astype(np.int64), t.astype(np.int64)


def remove_nodes(s, t, w, n, nodes, base=1):
    """transform.jl:212-252 -> (s2, t2, w2, n2, nid, eid): nid / eid the 0-based kept nodes / edge positions, ascending"""
    s, t = np.asarray(s, np.int64), np.asarray(t, np.int64)
    gone = np.zeros(n, bool)
    gone[np.asarray(sorted(set(int(v) for v in nodes)), np.int64) - base] = True     # sort(union(nodes_to_remove))
    keep_e = ~(gone[s - base] | gone[t - base])
    new = np.cumsum(~gone) - 1                                                       # s[s .> node] .-= 1 for every removed node
    s2, t2 = new[s[keep_e] - base] + base, new[t[keep_e] - base] + base
    w2 = None if w is None else np.asarray(w)[keep_e]
    return s2, t2, w2, int((~gone).sum()), np.flatnonzero(~gone), np.flatnonzero(keep_e)


def remove_nodes_p(s, t, w, n, p, seed, base=1):
    """transform.jl:273-276 with the library's mask in place of rand() < p"""
    return remove_nodes(s, t, w, n, np.flatnonzero(~keep_mask(seed, p, n)) + base, base)


def add_edges(s, t, w, n, snew, tnew, wnew=None, base=1):
    """transform.jl:322-353 -> (s2, t2, w2, n2); the weight rule is cat_features (utils.jl:119-122): a missing side is ones"""
    s, t = np.asarray(s, np.int64), np.asarray(t, np.int64)
    snew, tnew = np.asarray(snew, np.int64), np.asarray(tnew, np.int64)
    assert len(snew) == len(tnew)
    if len(snew) == 0:
        return s, t, w, n
    assert snew.min() >= base and tnew.min() >= base
    if w is None and wnew is None:
        w2 = None
    else:
        w1 = np.ones(len(s), np.float32) if w is None else np.asarray(w, np.float32)
        w2 = np.concatenate([w1, np.ones(len(snew), np.float32) if wnew is None else np.asarray(wnew, np.float32)])
    n2 = max(int(snew.max()) + 1 - base, int(tnew.max()) + 1 - base, n)
    return np.concatenate([s, snew]), np.concatenate([t, tnew]), w2, n2


def add_nodes(n, k):
    """transform.jl:553-561: the edge list stays, the nodes n + 1 .. n + k are new"""
    return n + k


def perturb_edges(s, t, w, n, ratio, seed, base=1):
    """transform.jl:388-420 with the library's pair draw in place of the rejection loop (same distribution: uniform over s != t)"""
    assert 0 <= ratio <= 1, "perturb_ratio must be between 0 and 1"
    m = math.ceil(len(s) * ratio)
    if m == 0:
        return np.asarray(s, np.int64), np.asarray(t, np.int64), w, n
    assert n > 1, "Graph must contain at least 2 nodes to add edges"
    sn, tn = rand_pairs(seed, m, n)
    return add_edges(s, t, w, n, sn + base, tn + base, None, base)
