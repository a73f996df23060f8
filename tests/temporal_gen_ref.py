"""The float64 restatement of hyperbolic_graph and of the two temporal generators' trajectories (include/gnnmp.h,
"gnnmp_hyperbolic_graph_f32"; gnnmp/generate.py) that tests/test_temporal_generators.py and tests/test_hyperbolic_graph_abi.py compare
against, and the inputs of their GPU cases.  numpy only; rows are 0-based here.

The pair value is v = cosh(zeta (r_i - r_j)) + 2 sinh(zeta r_i) sinh(zeta r_j) sin^2((theta_i - theta_j) / 2), two non-negative terms:
the reference's own cosh cosh - sinh sinh cos (generate.jl:287-297, hyp_distance_literal below) cancels — at zeta R = 20 it is off by 1e-6
relative even in Float64 — and is only used here where it is accurate (zeta R <= 4).

B: the device evaluates 2 v = fmaf(F_i, E_j, E_i F_j) + (S_i S_j) h from per-node E, F, S (double, one fp32 rounding each: u = 2^-24) and
h (double chord, one fp32 rounding).  E_i F_j: 3 u; the fma on top: 4 u.  S_i S_j: 3 u; times h: 5 u.  The sum of the two positive terms:
6 u.  The threshold fl32(2 cosh(zeta R)): 1 u.  The double-precision work (sincos, exp, sinh within 2 ulp of double) stays below 1 u for
every pair this module makes (zeta (r_i + r_j) <= 40: S_i S_j 2^-50 sqrt(h) <= u v, include/gnnmp.h).  7 u + 1 u: B = 8, never fitted to
device output.  The band of the issue carries the factor (1 + zeta R) on top of it; the device bound does not need it."""
import numpy as np

U = 2.0 ** -24
B = 8.0
BAND_CAP = 1e-3                        # at most this fraction of the ordered pairs i != j may lie in the band

NS = (1, 15, 16, 17, 63, 64, 65, 129, 257)          # 16 queries a block, 64 candidates a tile
ZETAS = (0.7, 1.0, 2.0)
ZETA_RS = (1.0, 4.0, 10.0, 20.0)


def f32(v):
    """the float32 the device receives, as a Python float"""
    return float(np.float32(v))


def hyp_v(points, zeta, rows=None):
    """(len(rows), N) float64 values v(i, j) in the cancellation-free form"""
    p = np.asarray(points, np.float64)
    rows = np.arange(p.shape[0]) if rows is None else np.asarray(rows, np.int64)
    r, th = p[:, 0], p[:, 1]
    with np.errstate(invalid="ignore", over="ignore"):
        half = np.sin((th[rows][:, None] - th[None, :]) / 2.0)
        return np.cosh(zeta * (r[rows][:, None] - r[None, :])) + 2.0 * np.sinh(zeta * r[rows])[:, None] * np.sinh(zeta * r)[None, :] * half * half


def hyp_distance(a, b, zeta):
    """the hyperbolic distance of two points (r, theta) through the cancellation-free value"""
    if tuple(a) == tuple(b):
        return 0.0
    return float(np.arccosh(max(1.0, hyp_v(np.array([a, b], np.float64), zeta, rows=[0])[0, 1])) / zeta)


def hyp_distance_literal(a, b, zeta):
    """_hyperbolic_distance (generate.jl:287-297) restated literally"""
    if tuple(a) == tuple(b):
        return 0.0
    ca = np.cosh(zeta * a[0]) * np.cosh(zeta * b[0])
    cb = np.sinh(zeta * a[0]) * np.sinh(zeta * b[0])
    cc = np.cos(np.pi - abs(np.pi - abs(a[1] - b[1])))
    return float(np.arccosh(ca - cb * cc) / zeta)


def candidates(N, gi, self_loops):
    """(N, N) bool: j is a candidate of i (same graph; j != i without self loops)"""
    ok = np.ones((N, N), bool) if gi is None else (np.asarray(gi)[:, None] == np.asarray(gi)[None, :])
    if not self_loops:
        ok = ok & ~np.eye(N, dtype=bool)
    return ok


def hyp_adjacency(points32, R, zeta, gi=None, self_loops=False):
    """(adj, band): adj[i, j] = j is a neighbour of centre i, evaluated in float64 on the float32 points with the float32 R and zeta
    the device receives; band[i, j] = the pair lies within B (1 + zeta R) 2^-24 cosh(zeta R) of the threshold (either answer is
    accepted there).  A node to itself has v = 1.  A value that is not finite is no edge."""
    pts = np.asarray(points32, np.float32)
    N = pts.shape[0]
    z, Rf = f32(zeta), f32(R)
    C = np.cosh(z * Rf)
    v = hyp_v(pts, z)
    v[np.arange(N), np.arange(N)] = np.where(np.isfinite(pts).all(1), 1.0, np.nan)
    ok = candidates(N, gi, self_loops)
    with np.errstate(invalid="ignore"):
        adj = ok & np.isfinite(v) & (v <= C)
        band = ok & ~np.eye(N, dtype=bool) & (np.abs(v - C) <= B * (1.0 + z * Rf) * U * C)
    return adj, band


def band_fraction(band, gi=None):
    N = band.shape[0]
    pairs = N * (N - 1)
    return 0.0 if pairs == 0 else float(band.sum()) / pairs


def adjacency_coo(adj, base=1):
    """GNNGraph(adj) of a symmetric dense adjacency (convert.jl:75-95, column-major findall): targets ascend, sources ascend within a
    target — the plan's order with dir = :in"""
    t, s = np.nonzero(adj)             # row-major over (centre, neighbour) = column-major over (source, target) of the symmetric matrix
    return s.astype(np.int64) + base, t.astype(np.int64) + base


# ---- the trajectories -------------------------------------------------------------------------------------------------------------------
def radius_trajectory(u0, u_rho, u_theta, speed):
    """[T, N, 2] float64 (generate.jl:272-281): point by point, step by step"""
    pos = np.array(u0, np.float64)
    out = [pos.copy()]
    for k in range(len(u_rho)):
        for i in range(pos.shape[0]):
            rho = 2.0 * speed * u_rho[k][i] - speed
            th = 2.0 * np.pi * u_theta[k][i]
            pos[i, 0] = 1.0 - abs(1.0 - abs(pos[i, 0] + rho * np.cos(th)))
            pos[i, 1] = 1.0 - abs(1.0 - abs(pos[i, 1] + rho * np.sin(th)))
        out.append(pos.copy())
    return np.stack(out)


def hyperbolic_trajectory(u_p, u_theta0, u_dp, u_dtheta, alpha, R, speed):
    """([T, N, 2] float64 rows (r, theta), [T, N] the quantiles p) (generate.jl:351-377)"""
    p = np.array(u_p, np.float64)
    th = 2.0 * np.pi * np.array(u_theta0, np.float64)
    radius = lambda q: np.arccosh(1.0 + (np.cosh(alpha * R) - 1.0) * q) / alpha
    out, ps = [], []
    for k in range(len(u_dp) + 1):
        out.append(np.stack([radius(p), th], axis=-1))
        ps.append(p.copy())
        if k < len(u_dp):
            p = p + (2.0 * speed * np.asarray(u_dp[k], np.float64) - speed)
            hi = p > 1.0
            p[hi] = 1.0 - np.fmod(p[hi], 1.0)
            lo = p < 0.0
            p[lo] = np.abs(p[lo])
            th = th + (2.0 * speed * np.asarray(u_dtheta[k], np.float64) - speed)
    return np.stack(out), np.stack(ps)


# ---- the inputs of the GPU cases ---------------------------------------------------------------------------------------------------------
def hyp_points(rng, n, R, alpha=1.0):
    """n float32 points of the disk of radius R, quasi-uniform as the generator makes them; theta drifted below 0 and above 2 pi; and,
    where n allows: a node at r = 0, a duplicated point, and two points within 1e-4 of each other across the 0 / 2 pi seam"""
    p = rng.random(n)
    r = np.arccosh(1.0 + (np.cosh(alpha * R) - 1.0) * p) / alpha
    th = rng.uniform(-2.0 * np.pi, 4.0 * np.pi, n)
    pts = np.stack([r, th], axis=-1).astype(np.float32)
    if n >= 6:
        pts[1, 0] = 0.0                                             # the origin
        pts[3] = pts[2]                                             # a duplicate
        pts[4] = (pts[2, 0], 4e-5)                                  # the seam, from both sides
        pts[5] = (pts[2, 0], np.float32(2.0 * np.pi - 5e-5))
    return pts


class HypCase:
    def __init__(self, name, points, zeta, R, gi, ib, base, loops, n_graphs):
        self.name, self.points, self.zeta, self.R, self.gi, self.ib, self.base, self.loops, self.n_graphs = \
            name, points, zeta, R, gi, ib, base, loops, n_graphs

    def __repr__(self):
        return self.name


def hyp_cases():
    """every hyperbolic input of the GPU tests: the point counts of NS alone, a batch of segments (1, 17, 64, 3) and one of 5 x 30 (blocks
    straddle the segments), each with a sorted and an unsorted indicator; index widths, bases, self loops, zeta and zeta R cycle"""
    cases, n = [], 0

    def add(name, sizes, mode, forms=None):
        nonlocal n
        zeta, zr = ZETAS[n % 3], ZETA_RS[n % 4]
        loops, ib, base = forms or (bool(n % 2), (8, 4)[(n // 2) % 2], (1, 0)[(n // 4) % 2])
        rng = np.random.default_rng(500 + n)
        N = sum(sizes)
        R = zr / zeta
        pts = hyp_points(rng, N, R, alpha=zeta)
        gi = None
        if mode != "none":
            gi = np.repeat(np.arange(len(sizes)), sizes)
            if mode == "unsorted":
                gi = rng.permutation(gi)
        cases.append(HypCase(f"{name}-z{zeta}-zR{zr}-ib{ib}-b{base}-{'loops' if loops else 'noloops'}", pts, zeta, R, gi, ib, base, loops,
                             len(sizes)))
        n += 1

    for N in NS:
        add(f"N{N}", [N], "none")
    for zr_round in range(3):                                       # N = 129 once more under the other index forms and zeta R
        add(f"N129r{zr_round}", [129], "none")
    add("segs-sorted", [1, 17, 64, 3], "sorted", (False, 8, 1))
    add("5x30-sorted", [30] * 5, "sorted", (True, 4, 1))
    add("segs-unsorted", [1, 17, 64, 3], "unsorted", (True, 4, 0))
    add("5x30-unsorted", [30] * 5, "unsorted", (False, 8, 0))
    cases.append(seam_case())
    return cases


def seam_case(zeta=1.0, R=20.0, pairs=8):
    """pairs of points within 1e-4 of each other across the 0 / 2 pi seam whose value lies 3 % below (even pairs) or above (odd pairs)
    the threshold: an angular difference formed in float32 is off by up to 5 % there and flips them"""
    C = np.cosh(zeta * R)
    pts = []
    for k in range(pairs):
        ta, tb = 1e-5 * (k + 1), 2.0 * np.pi - 6e-5
        half = np.sin((tb - ta) / 2.0)
        target = C * (0.97 if k % 2 == 0 else 1.03)
        r = np.arcsinh(np.sqrt((target - 1.0) / 2.0) / abs(half)) / zeta
        pts += [(r, ta), (r, tb)]
    return HypCase("seam-z1.0-zR20.0", np.array(pts, np.float32), zeta, R, np.repeat(np.arange(pairs), 2), 8, 1, False, pairs)


_CASES = None


def cases():
    global _CASES
    if _CASES is None:
        _CASES = hyp_cases()
    return _CASES


_ADJ = {}


def case_adjacency(c):
    """(adj, band) of a case, computed once and shared"""
    if c.name not in _ADJ:
        _ADJ[c.name] = hyp_adjacency(c.points, c.R, c.zeta, c.gi, c.loops)
    return _ADJ[c.name]
