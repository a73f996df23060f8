"""The cell-grid route of radius_graph (csrc/neighbors_grid.hip, planned by csrc/neighbors_route.h): the same plan as the brute search, bit
for bit.  Points on a dyadic lattice (multiples of 2^-4, |x| <= 32) make float32 and float64 agree exactly, so the float64 restatement of
tests/neighbors_ref.py is THE answer and ties d2 == r2 are real: rowptr, col and eid must be equal to it.  On arbitrary floats the
reference is the brute route of the same build."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import neighbors_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
gpu = pytest.mark.gpu
HOOKS = ("gnnmp_debug_neighbors_route", "gnnmp_debug_neighbors_force")
ROW_CAP = 1024                                   # csrc/neighbors_route.h: NB_GRID_ROW_CAP
SIZES = (1, 700, 0, 37, 1300)                    # a sorted indicator: a single node, a graph id that does not occur


def test_hooks_in_header_symbols_and_library_and_the_planner_is_plain_cpp():
    from gnnmp import _lib
    header = open(os.path.join(ROOT, "include", "gnnmp.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    for name in HOOKS:
        assert name in _lib.SYMBOLS and name in exported
        assert header.index("GNNMP_INTERNAL") < header.index(f"int {name}(")
    lib = _lib.load()
    assert lib.gnnmp_debug_neighbors_route(None) == _lib.EINVAL
    assert lib.gnnmp_debug_neighbors_force(3) == _lib.EINVAL and lib.gnnmp_debug_neighbors_force(0) == _lib.OK
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "graphneuralnetworks.jl_amd", "csrc"),
                    "-include", "neighbors_route.h", "-x", "c++", os.devnull], check=True)


def _points(kind, d, n, rng):
    """(x float32 on the lattice, r): `span` lattice steps an axis keep about one point a lattice site at n = 2 000"""
    span = {1: 512, 2: 64, 3: 16}[d]
    x = (rng.integers(0, span, (n, d)) / 16.0).astype(np.float32)
    if kind == "cutoff":            # r = one lattice step: hits sit exactly on the cutoff and in the next cell
        return x, 1.0 / 16.0
    if kind == "duplicates":        # a few sites, r = 0: only coincident points are neighbours
        return (rng.integers(0, 8, (n, d)) / 16.0).astype(np.float32), 0.0
    if kind == "negative":
        return x - np.float32(32.0), 1.0 / 16.0
    if kind == "nonfinite":         # degree 0 and no loop for the three, nothing else moves
        x[5, 0], x[9, d - 1], x[n - 2, 0] = np.nan, np.inf, -np.inf
        return x, 2.0 / 16.0
    if kind == "outlier":           # the box is 1e30 wide: the cell side grows, the answer does not change
        x[7] = np.float32(1e30)
        return x, 2.0 / 16.0
    assert kind == "onecell"        # r beyond the extent: every point of a graph is a neighbour
    return x, 100.0


def _plan_arrays(g):
    rowptr, col, eid = g._plans[False].export64()
    return rowptr.cpu().numpy(), col.cpu().numpy(), eid.cpu().numpy()


@gpu
@pytest.mark.parametrize("loops", [0, 1])
@pytest.mark.parametrize("indicator", [False, True])
@pytest.mark.parametrize("d", [1, 2, 3])
@pytest.mark.parametrize("kind", ["cutoff", "duplicates", "negative", "nonfinite", "outlier", "onecell"])
def test_grid_equals_the_float64_reference_on_the_lattice(kind, d, indicator, loops):
    import torch
    import gnnmp
    from gnnmp import neighbors as NB
    sizes = tuple(s // 3 for s in SIZES) if kind == "onecell" else SIZES        # (rows stay below the row cap: the grid writes)
    n = sum(sizes)
    x, r = _points(kind, d, n, np.random.default_rng(100 * d + len(kind)))
    gi = np.repeat(np.arange(len(sizes)), sizes) if indicator else None
    g = gnnmp.radius_graph(torch.from_numpy(x).cuda(), r, None if gi is None else torch.from_numpy(gi + 1).cuda(),
                           self_loops=bool(loops), route="grid")
    assert NB.last_route()[0] == NB.ROUTE_GRID
    lists = R.radius_ref(x, np.float64(np.float32(r) * np.float32(r)), gi, bool(loops))
    _, _, ref_rowptr = R.radius_coo(lists)
    rowptr, col, eid = _plan_arrays(g)
    assert np.array_equal(rowptr, ref_rowptr)
    assert np.array_equal(col, np.concatenate(lists)) and np.array_equal(eid, np.arange(len(col)))
    if kind == "nonfinite":
        assert all(len(lists[i]) == 0 for i in (5, 9, n - 2))


def _same_plan(a, b):
    import torch
    pa, pb = a._plans[False], b._plans[False]
    assert (pa.n_total, pa.max_degree, pa.n_long, pa.long_thresh) == (pb.n_total, pb.max_degree, pb.n_long, pb.long_thresh)
    assert all(torch.equal(u, v) for u, v in zip(pa.export64(), pb.export64()))


@gpu
@pytest.mark.parametrize("r", [0.25, 0.9])
def test_grid_equals_brute_on_arbitrary_floats_and_reruns(r):
    import torch
    import gnnmp
    x = torch.randn((4096, 3), device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
    brute, grid, again = (gnnmp.radius_graph(x, r, route=rt) for rt in ("brute", "grid", "grid"))
    assert brute.num_edges > 4096
    _same_plan(grid, brute)
    _same_plan(again, grid)


@gpu
def test_a_row_above_the_cap_is_written_by_the_brute_kernel():
    import torch
    import gnnmp
    from gnnmp import neighbors as NB
    x = torch.rand((1024 + ROW_CAP + 100, 3), device="cuda", generator=torch.Generator(device="cuda").manual_seed(4))
    x[500:500 + ROW_CAP + 100] = x[500].clone()                           # cap + 100 coincident points inside 1 k others
    grid = gnnmp.radius_graph(x, 0.05, route="grid")
    info = NB.last_route()
    assert info[0] == NB.ROUTE_GRID_COUNT_BRUTE_WRITE and info[5] == 9 and info[4] >= ROW_CAP + 100
    _same_plan(grid, gnnmp.radius_graph(x, 0.05, route="brute"))


@gpu
@pytest.mark.parametrize("what", ["d4", "unsorted"])
def test_a_forced_grid_is_refused_where_it_cannot_run(what):
    import torch
    import gnnmp
    from gnnmp import _lib as L, neighbors as NB
    x = torch.rand((300, 4 if what == "d4" else 3), device="cuda")
    gi = None if what == "d4" else (torch.arange(300, device="cuda") % 3 + 1)
    with pytest.raises(L.GnnmpError) as e:
        gnnmp.radius_graph(x, 0.2, gi, route="grid")
    assert e.value.status == L.EUNSUPPORTED and "grid" in str(e.value)
    h = ctypes.c_void_p(0x1)                                              # at the ABI: *out is NULL after the refusal
    lib = L.load()
    lib.gnnmp_debug_neighbors_force(2)
    try:
        rc = lib.gnnmp_radius_graph_f32(ctypes.byref(h), L.ptr(x), 300, x.shape[1], ctypes.c_float(0.2), L.ptr(gi), 8, 1, 3, 0, L.stream_ptr())
    finally:
        lib.gnnmp_debug_neighbors_force(0)
    assert rc == L.EUNSUPPORTED and not h.value
    gnnmp.radius_graph(x, 0.2, gi)                                        # the route was put back: auto, and this shape is brute
    assert NB.last_route()[0] == NB.ROUTE_BRUTE


@gpu
def test_auto_takes_the_grid_on_a_large_cloud_and_the_brute_search_on_a_small_one():
    import torch
    import gnnmp
    from gnnmp import neighbors as NB
    x = torch.rand((131072, 3), device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    r = 0.0331                                                            # 4/3 pi r^3 N = 20 neighbours
    auto = gnnmp.radius_graph(x, r)
    info = NB.last_route()
    assert info[0] == NB.ROUTE_GRID and min(info[1:4]) >= 16 and info[5] == 0
    assert 15 * 131072 < auto.num_edges < 25 * 131072
    _same_plan(auto, gnnmp.radius_graph(x, r, route="brute"))             # 1.7e10 pair tests, once
    gnnmp.radius_graph(x[:1024], 0.1)
    assert NB.last_route()[0] == NB.ROUTE_BRUTE and NB.last_route()[5] == 6
