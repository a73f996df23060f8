"""The float64 brute-force restatement of knn_graph / radius_graph (include/gnnmp.h, "Neighbour search") that the neighbour tests
and the memory-contract table compare against.  numpy only; rows are 0-based here."""
import numpy as np


def sqdist_rows(x, rows):
    """(len(rows), N) float64 squared distances, accumulated over the dimensions in order; non-finite -> +inf"""
    x = np.asarray(x, np.float64)
    rows = np.asarray(rows, np.int64)
    d2 = np.zeros((len(rows), x.shape[0]), np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(x.shape[1]):
            diff = x[rows, c][:, None] - x[None, :, c]
            d2 += diff * diff
    d2[~np.isfinite(d2)] = np.inf
    return d2


def _candidates(i, N, gi, self_loops):
    ok = np.ones(N, bool) if gi is None else (gi == gi[i])
    if not self_loops:
        ok = ok.copy()
        ok[i] = False
    return ok


def knn_ref(x, k, gi=None, self_loops=False, rows=None, chunk=256):
    """(nbr, d2): nbr[a, r] = the r-th candidate of node rows[a] in the order (d2, j); d2 the float64 distances of those"""
    x = np.asarray(x)
    N = x.shape[0]
    rows = np.arange(N) if rows is None else np.asarray(rows, np.int64)
    gi = None if gi is None else np.asarray(gi, np.int64)
    nbr = np.zeros((len(rows), k), np.int64)
    dk = np.zeros((len(rows), k), np.float64)
    for c0 in range(0, len(rows), chunk):
        rr = rows[c0:c0 + chunk]
        d2 = sqdist_rows(x, rr)
        for a, i in enumerate(rr):
            row = np.where(_candidates(i, N, gi, self_loops), d2[a], np.nan)   # nan = not a candidate
            cand = np.flatnonzero(~np.isnan(row))
            assert len(cand) >= k, "a graph with fewer candidates than k"
            vals = row[cand]
            kth = np.partition(vals, k - 1)[k - 1]
            keep = cand[vals <= kth]
            order = keep[np.argsort(row[keep], kind="stable")][:k]                # stable: ties in ascending j
            nbr[c0 + a] = order
            dk[c0 + a] = row[order]
    return nbr, dk


def radius_ref(x, r2, gi=None, self_loops=False):
    """list over the nodes of the ascending neighbour arrays with d2 <= r2"""
    x = np.asarray(x)
    N = x.shape[0]
    gi = None if gi is None else np.asarray(gi, np.int64)
    out = []
    for c0 in range(0, N, 256):
        rr = np.arange(c0, min(N, c0 + 256))
        d2 = sqdist_rows(x, rr)
        for a, i in enumerate(rr):
            out.append(np.flatnonzero(_candidates(i, N, gi, self_loops) & (d2[a] <= r2)))
    return out


def knn_coo(nbr, dir_out=False, base=1, rows=None):
    """adjacency list -> COO (convert.jl:97-117): edge i k + r joins centre i and nbr[i, r]"""
    n, k = nbr.shape
    centre = np.repeat(np.arange(n) if rows is None else np.asarray(rows), k)
    nb = nbr.reshape(-1)
    s, t = (centre, nb) if dir_out else (nb, centre)
    return s + base, t + base


def radius_coo(lists, dir_out=False, base=1):
    deg = np.array([len(v) for v in lists], np.int64)
    rowptr = np.concatenate([[0], np.cumsum(deg)])
    centre = np.repeat(np.arange(len(lists)), deg)
    nb = np.concatenate(lists) if len(lists) else np.zeros(0, np.int64)
    s, t = (centre, nb) if dir_out else (nb, centre)
    return s.astype(np.int64) + base, t.astype(np.int64) + base, rowptr


def grid_points(rng, n, d, span=4):
    """points on a small integer grid: every fp32 step of the distance is exact, and ties abound"""
    return rng.integers(0, span, (n, d)).astype(np.float32)
