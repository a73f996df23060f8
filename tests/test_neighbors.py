"""knn_graph / radius_graph on the device (csrc/neighbors.hip, gnnmp/neighbors.py) against the float64 brute-force restatement of
tests/neighbors_ref.py.  Exact cases (integer grid: every fp32 step exact, ties everywhere) are compared element for element; random
cases node by node, where a node may differ from float64 only inside the tie band: every index of the symmetric difference has a
float64 distance within 1e-5 relative of the float64 k-th distance (of r for radius_graph) — the project's parity bar, applied to the
only place where fp32 rounding can show."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import neighbors_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
BAND = 1e-5
DS = (1, 2, 3, 8, 64, 100)
KS = (1, 3, 16, 17, 64, 65, 200)


def _torch():
    import torch
    import gnnmp
    return torch, gnnmp


def _cpu(v):
    return v.cpu().numpy().astype(np.int64)


def _segments(need, n_seg=3):
    """unequal graph sizes, one of exactly `need` nodes; the total is no multiple of a tile"""
    sizes = [need + 37, need, 2 * need + 5][:n_seg]
    if sum(sizes) % 16 == 0:
        sizes[0] += 1
    return sizes


def _indicator(rng, sizes, mode):
    if mode == "none":
        return None
    gi = np.repeat(np.arange(len(sizes)), sizes)
    return rng.permutation(gi) if mode == "unsorted" else gi


def _exact_combos():
    n = 0
    for d in DS:
        for k in KS:
            yield (d, k, ("in", "out")[n % 2], bool((n // 2) % 2), (8, 4)[(n // 4) % 2], (1, 0)[(n // 8) % 2],
                   ("sorted", "unsorted", "none")[n % 3])
            n += 1


@pytest.mark.parametrize("d,k,dir,loops,ib,base,mode", list(_exact_combos()))
def test_knn_exact(d, k, dir, loops, ib, base, mode):
    torch, gnnmp = _torch()
    rng = np.random.default_rng(1000 * d + k)
    need = k + (0 if loops else 1)
    sizes = _segments(need)
    N = sum(sizes)
    x = R.grid_points(rng, N, d)
    gi = _indicator(rng, sizes, mode)
    dt = torch.int64 if ib == 8 else torch.int32
    g = gnnmp.knn_graph(torch.from_numpy(x).cuda(), k, None if gi is None else torch.from_numpy(gi + base).cuda(), self_loops=loops,
                        dir=dir, index_base=base, idx_dtype=dt)
    s, t = R.knn_coo(R.knn_ref(x, k, gi, loops)[0], dir == "out", base)
    assert g.s.dtype == dt and g.num_nodes == N and g.num_edges == N * k
    assert g.num_graphs == (1 if gi is None else len(sizes))
    assert np.array_equal(_cpu(g.s), s) and np.array_equal(_cpu(g.t), t)


@pytest.mark.parametrize("d,mode,loops,dir,ib,base", [(1, "sorted", False, "in", 8, 1), (2, "none", True, "out", 4, 0), (3, "unsorted", False, "in", 4, 1),
                                                      (8, "sorted", True, "in", 8, 0), (64, "none", False, "out", 8, 1), (100, "unsorted", True, "in", 4, 0)])
def test_radius_exact(d, mode, loops, dir, ib, base):
    torch, gnnmp = _torch()
    rng = np.random.default_rng(77 + d)
    sizes = _segments(20)
    N = sum(sizes)
    x = R.grid_points(rng, N, d)
    gi = _indicator(rng, sizes, mode)
    r = float(np.sqrt(np.float32(max(1, (5 * d) // 2))))               # r^2 = the grid's mean d2, an integer up to rounding: a boundary full of ties
    r2 = float(np.float32(r) * np.float32(r))
    dt = torch.int64 if ib == 8 else torch.int32
    g = gnnmp.radius_graph(torch.from_numpy(x).cuda(), r, None if gi is None else torch.from_numpy(gi + base).cuda(), self_loops=loops,
                           dir=dir, index_base=base, idx_dtype=dt)
    s, t, _ = R.radius_coo(R.radius_ref(x, r2, gi, loops), dir == "out", base)
    assert g.num_edges == len(s) and len(s) > 0
    assert np.array_equal(_cpu(g.s), s) and np.array_equal(_cpu(g.t), t)


def test_single_node_and_empty():
    torch, gnnmp = _torch()
    x = torch.zeros((1, 3), device="cuda")
    g = gnnmp.knn_graph(x, 1, self_loops=True)
    assert _cpu(g.s).tolist() == [1] and _cpu(g.t).tolist() == [1]
    with pytest.raises(AssertionError):
        gnnmp.knn_graph(x, 1)                                   # one node, no self loops: fewer than k + 1 points
    assert gnnmp.radius_graph(x, 1.0).num_edges == 0
    assert gnnmp.radius_graph(x, 1.0, self_loops=True).num_edges == 1
    assert gnnmp.knn_graph(torch.zeros((0, 3), device="cuda"), 2).num_edges == 0


def test_errors_like_the_reference():
    torch, gnnmp = _torch()
    x = torch.rand((20, 3), device="cuda")
    gi = torch.tensor([1] * 17 + [2] * 3, device="cuda")
    with pytest.raises(AssertionError):
        gnnmp.knn_graph(x, 3, gi)                               # @assert all(values(cm) .>= k): graph 2 has 3 < k + 1 nodes
    assert gnnmp.knn_graph(x, 3, gi, self_loops=True).num_edges == 60
    with pytest.raises(AssertionError):
        gnnmp.knn_graph(x, 3, gi[torch.randperm(20, device="cuda")])   # the same through an unsorted indicator
    with pytest.raises(AssertionError):
        gnnmp.knn_graph(x, 3, gi[:19])                          # @assert length(graph_indicator) == n
    with pytest.raises(AssertionError):
        gnnmp.knn_graph(x, 3, gi.float())                       # @assert graph_indicator isa AbstractVector{<:Integer}
    with pytest.raises(AssertionError):
        gnnmp.knn_graph(x, 3, dir="both")
    with pytest.raises(ValueError):
        gnnmp.knn_graph(x, 1025)
    with pytest.raises(ValueError):
        gnnmp.radius_graph(x, float("nan"))
    # an id that skips a graph is fine (countmap holds only the ids that occur); num_graphs = maximum(graph_indicator)
    gi3 = torch.tensor([1] * 10 + [3] * 10, device="cuda")
    assert gnnmp.knn_graph(x, 3, gi3).num_graphs == 3


# ---- random points: every node, the tie band ------------------------------------------------------------------------------------------
def _band_check_knn(x, k, gi, loops, nbr_gpu, rows=None):
    """nodes that needed the band; asserts the rule for every node"""
    rows = np.arange(x.shape[0]) if rows is None else rows
    ref, dref = R.knn_ref(x, k, gi, loops, rows=rows)
    needed = 0
    for c0 in range(0, len(rows), 256):
        rr = rows[c0:c0 + 256]
        d2 = R.sqdist_rows(x, rr)
        for a, i in enumerate(rr):
            got = nbr_gpu[c0 + a]
            kth = dref[c0 + a, k - 1]
            assert len(set(got.tolist())) == k and (loops or i not in got)
            if gi is not None:
                assert np.all(gi[got] == gi[i])
            dg = d2[a, got]
            assert np.all(np.diff(dg) >= -BAND * kth), f"node {i}: distances not non-decreasing"
            diff = np.setxor1d(got, ref[c0 + a])
            if len(diff):
                needed += 1
                assert np.all(np.abs(d2[a, diff] - kth) <= BAND * kth), f"node {i}: outside the tie band"
    return needed


@pytest.mark.parametrize("d", [3, 64])
def test_knn_random_every_node(d):
    torch, gnnmp = _torch()
    rng = np.random.default_rng(d)
    N, k = 4096, 16
    x = rng.random((N, d), dtype=np.float32)
    for gi in (None, np.repeat(np.arange(4), [1000, 24, 2048, 1024])):
        g = gnnmp.knn_graph(torch.from_numpy(x).cuda(), k, None if gi is None else torch.from_numpy(gi + 1).cuda())
        assert np.array_equal(_cpu(g.t), np.repeat(np.arange(N), k) + 1)
        needed = _band_check_knn(x, k, gi, False, (_cpu(g.s) - 1).reshape(N, k))
        print(f"knn random d={d} indicator={'no' if gi is None else 'yes'}: {needed} of {N} nodes needed the tie band")


@pytest.mark.parametrize("d", [3, 64])
def test_radius_random_every_node(d):
    torch, gnnmp = _torch()
    rng = np.random.default_rng(10 + d)
    N = 4096
    x = rng.random((N, d), dtype=np.float32)
    r = 0.12 if d == 3 else 2.9
    r2 = float(np.float32(r) * np.float32(r))
    g = gnnmp.radius_graph(torch.from_numpy(x).cuda(), r)
    s, t = _cpu(g.s) - 1, _cpu(g.t) - 1
    assert np.all(np.diff(t) >= 0)
    ref = R.radius_ref(x, r2)
    bounds = np.searchsorted(t, np.arange(N + 1))
    needed = 0
    for c0 in range(0, N, 256):
        d2 = R.sqdist_rows(x, np.arange(c0, min(N, c0 + 256)))
        for a in range(d2.shape[0]):
            i = c0 + a
            got = s[bounds[i]:bounds[i + 1]]
            assert np.all(np.diff(got) > 0)
            diff = np.setxor1d(got, ref[i])
            if len(diff):
                needed += 1
                assert np.all(np.abs(np.sqrt(d2[a, diff]) - r) <= BAND * r), f"node {i}: outside the band at the boundary"
    assert g.num_edges > N
    print(f"radius random d={d}: {needed} of {N} nodes needed the boundary band; {g.num_edges} edges")


def test_rerun_is_bit_identical():
    torch, gnnmp = _torch()
    x = torch.rand((5000, 5), device="cuda")
    gi = torch.sort(torch.randint(1, 6, (5000,), device="cuda"))[0]
    a, b = gnnmp.knn_graph(x, 70, gi), gnnmp.knn_graph(x, 70, gi)
    assert torch.equal(a.s, b.s) and torch.equal(a.t, b.t)
    a, b = gnnmp.radius_graph(x, 0.3, gi), gnnmp.radius_graph(x, 0.3, gi)
    assert torch.equal(a.s, b.s) and torch.equal(a.t, b.t) and a.num_edges > 0


def test_properties_on_a_large_cloud():
    """the reference's test items (GNNGraphs/test/generate.jl:39-81) at 10^5 points"""
    torch, gnnmp = _torch()
    n, k = 100_000, 8
    x = torch.rand((n, 3), device="cuda")
    g = gnnmp.knn_graph(x, k)
    assert g.num_edges == n * k
    assert torch.all(gnnmp.degree(g, dir="in") == k)
    assert not gnnmp.has_self_loops(g)
    g = gnnmp.knn_graph(x, k, dir="out", self_loops=True)
    assert torch.all(gnnmp.degree(g, dir="out") == k)
    assert gnnmp.has_self_loops(g)
    gi = torch.sort(torch.randint(1, 9, (n,), device="cuda"))[0]
    g = gnnmp.knn_graph(x, k, gi)
    assert g.num_graphs == 8 and torch.all(gnnmp.degree(g, dir="in") == k)
    assert torch.equal(gi[g.s - 1], gi[g.t - 1])                 # no edge crosses the graphs
    g = gnnmp.radius_graph(x, 0.02, gi)
    assert not gnnmp.has_self_loops(g) and torch.equal(gi[g.s - 1], gi[g.t - 1])


def test_non_finite_rows_rank_last():
    torch, gnnmp = _torch()
    rng = np.random.default_rng(3)
    N, k = 200, 7
    x = R.grid_points(rng, N, 3, span=6)
    clean, _ = R.knn_ref(x, k)
    bad = x.copy()
    bad[50] = np.nan
    bad[120, 1] = np.inf
    g = gnnmp.knn_graph(torch.from_numpy(bad).cuda(), k)
    nbr = (_cpu(g.s) - 1).reshape(N, k)
    assert nbr.min() >= 0 and nbr.max() < N
    assert torch.all(gnnmp.degree(g, dir="in") == k)
    assert np.array_equal(nbr, R.knn_ref(bad, k)[0])             # the bad rows rank as +inf, ties by index
    untouched = ~np.isin(clean, (50, 120)).any(axis=1)
    untouched[[50, 120]] = False
    assert untouched.sum() > N // 2 and np.array_equal(nbr[untouched], clean[untouched])
    finite = np.setdiff1d(np.arange(N), (50, 120))
    assert not np.isin(nbr[finite], (50, 120)).any()             # more than k finite candidates: a bad row is nobody's neighbour
    g = gnnmp.radius_graph(torch.from_numpy(bad).cuda(), 2.0)
    assert not np.isin(_cpu(g.s) - 1, (50, 120)).any() and not np.isin(_cpu(g.t) - 1, (50, 120)).any()


def test_the_plan_comes_for_free():
    """dir = :in: the graph is handed its plan without a sort, equal to the plan gnnmp_plan_create builds from the same (s, t)"""
    torch, gnnmp = _torch()
    x = torch.rand((3000, 3), device="cuda")
    gi = torch.sort(torch.randint(1, 4, (3000,), device="cuda"))[0]
    feats = torch.randn((3000, 24), device="cuda")
    for g in (gnnmp.knn_graph(x, 9, gi), gnnmp.knn_graph(x, 9, idx_dtype=torch.int32, index_base=0), gnnmp.radius_graph(x, 0.08, gi),
              gnnmp.radius_graph(x, 0.08, idx_dtype=torch.int32)):
        assert False in g._plans                                 # attached by the constructor
        free = g._plans[False]
        sorted_plan = gnnmp.Plan(g.s, g.t, g.num_nodes, g.num_nodes, g.index_base, False)
        (rp, col, eid), (rp2, col2, eid2) = free.export(), sorted_plan.export()
        assert torch.equal(rp, rp2)
        # up to the order inside a row: (row, col, eid) triples as sets — here the orders coincide as well (both keep edge order)
        assert torch.equal(col, col2) and torch.equal(eid, eid2)
        g2 = gnnmp.GNNGraph(g.s, g.t, num_nodes=g.num_nodes, index_base=g.index_base)
        y1 = gnnmp.propagate(gnnmp.copy_xj, g, "max", xj=feats)
        y2 = gnnmp.propagate(gnnmp.copy_xj, g2, "max", xj=feats)
        assert torch.equal(y1, y2)
    assert False not in gnnmp.knn_graph(x, 9, dir="out")._plans   # the ordinary path


def test_dynamic_edgeconv_end_to_end():
    """knn_graph(x) -> EdgeConv -> knn_graph(h, graph_indicator) -> EdgeConv -> GlobalPool on 8 clouds, against the same layers on the
    graphs the restatement builds (forward, the 1e-5 bar)"""
    torch, gnnmp = _torch()
    rng = np.random.default_rng(11)
    sizes = [120, 100, 140, 96, 128, 111, 90, 133]
    N, k = sum(sizes), 10
    gi = np.repeat(np.arange(8), sizes)
    x = rng.random((N, 3), dtype=np.float32)
    xd, gid = torch.from_numpy(x).cuda(), torch.from_numpy(gi + 1).cuda()
    mlp = lambda i, o, seed: [gnnmp.Dense((i, o), "relu", seed=seed), gnnmp.Dense((o, o), seed=seed + 1)]
    c1, c2 = gnnmp.EdgeConv(mlp(6, 32, 1), aggr="max"), gnnmp.EdgeConv(mlp(64, 32, 3), aggr="max")
    pool = gnnmp.GlobalPool("mean")

    def graph_ref(pts):
        s, t = R.knn_coo(R.knn_ref(pts, k, gi)[0])
        return gnnmp.GNNGraph(torch.from_numpy(s).cuda(), torch.from_numpy(t).cuda(), num_nodes=N, graph_indicator=gid, num_graphs=8)

    g1 = gnnmp.knn_graph(xd, k, gid)
    h1 = c1(g1, xd)
    g2 = gnnmp.knn_graph(h1, k, gid)
    out = pool(g2, c2(g2, h1)).cpu().numpy().astype(np.float64)
    r1 = graph_ref(x)
    hr1 = c1(r1, xd)
    r2 = graph_ref(hr1.cpu().numpy())
    ref = pool(r2, c2(r2, hr1)).cpu().numpy().astype(np.float64)
    assert out.shape == (8, 32)
    assert np.linalg.norm(out - ref) <= 1e-5 * np.linalg.norm(ref)
    assert np.abs(out - ref).max() <= 1e-5 * np.abs(ref).max()


def test_full_size_cloud():
    """N = 262 144, d = 3, k = 16: an N x N fp32 matrix would be 275 GB — passing shows the workspace bound; 2 048 sampled nodes"""
    torch, gnnmp = _torch()
    rng = np.random.default_rng(5)
    N, k = 262_144, 16
    x = rng.random((N, 3), dtype=np.float32)
    torch.cuda.reset_peak_memory_stats()
    g = gnnmp.knn_graph(torch.from_numpy(x).cuda(), k, dir="out")
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() < (1 << 30)
    assert np.array_equal(_cpu(g.s), np.repeat(np.arange(N), k) + 1)
    rows = np.sort(rng.choice(N, 2048, replace=False))
    nbr = (_cpu(g.t) - 1).reshape(N, k)[rows]
    needed = _band_check_knn(x, k, None, False, nbr, rows=rows)
    print(f"full-size cloud: {needed} of 2048 sampled nodes needed the tie band")


@pytest.mark.parametrize("shift", [0, 4, 8, 16])
def test_memory_contract(shift):
    """In the manner of tests/test_abi_memory_contract.py (its slab, tests/abi_cases.py): the inputs of the search and the edge index read
    off its plan lie in ONE poisoned slab between guard bands.  Every output element is written, no byte outside the outputs changes
    (the const inputs come back bit for bit), and `points` / `graph_indicator` may start at any 4-byte boundary."""
    import ctypes
    import abi_cases as A
    torch, gnnmp = _torch()
    from gnnmp import _lib
    lib = _lib.load()
    rng = np.random.default_rng(9)
    sizes = [40, 6, 51]
    N, d, k = sum(sizes), 5, 5
    x = R.grid_points(rng, N, d)
    gi0 = np.repeat(np.arange(3), sizes)
    for which, ib, base in (("knn", 8, 1), ("knn", 4, 0), ("radius", 4, 1), ("radius", 8, 0)):
        dt = np.int64 if ib == 8 else np.int32
        if which == "knn":
            s, t = R.knn_coo(R.knn_ref(x, k, gi0, False)[0], False, base)
        else:
            r = 3.0
            s, t, _ = R.radius_coo(R.radius_ref(x, 9.0, gi0, False), False, base)
        arrs = [A.Arr("points", "in", x), A.Arr("graph_indicator", "in", (gi0 + base).astype(dt)),
                A.Arr("out_src", "out", shape=(len(s),), dtype=dt), A.Arr("out_dst", "out", shape=(len(s),), dtype=dt)]
        shifts = {a.name: shift for a in arrs if shift and shift % a.dtype.itemsize == 0}
        slab = A.Slab(arrs, "cuda", shifts)
        h = ctypes.c_void_p()
        if which == "knn":
            rc = lib.gnnmp_knn_graph_f32(ctypes.byref(h), slab.ptr("points"), N, d, k, slab.ptr("graph_indicator"), ib, base, 3, 0, None)
        else:
            rc = lib.gnnmp_radius_graph_f32(ctypes.byref(h), slab.ptr("points"), N, d, ctypes.c_float(r), slab.ptr("graph_indicator"),
                                            ib, base, 3, 0, None)
        assert rc == 0, lib.gnnmp_last_error()
        try:
            assert slab.check({}, untouched=True) == []          # the search itself writes nothing the caller owns
            info = (ctypes.c_int64 * 8)()
            assert lib.gnnmp_plan_info(h, info) == 0 and info[2] == len(s) and info[1] == N
            assert lib.gnnmp_plan_edge_index(h, ib, base, slab.ptr("out_src"), slab.ptr("out_dst"), None) == 0
            torch.cuda.synchronize()
            problems = slab.check({"out_src": A.E(s.astype(dt), "exact"), "out_dst": A.E(t.astype(dt), "exact")})
            assert problems == [], (which, ib, base, shift, problems)
        finally:
            lib.gnnmp_plan_destroy(h)
