"""gnnmp_hyperbolic_graph_f32 / gnnmp.hyperbolic_graph (csrc/neighbors.hip, gnnmp/generate.py) against the float64 restatement of
tests/temporal_gen_ref.py.

Without a GPU: the export is in header, SYMBOLS and library and owes no case to the memory-contract table; every refusal comes before
any HIP call and hands out no plan; the restatement agrees with the reference's own formula where that is accurate; and the BAND
condition holds for every input of the GPU cases — the pairs whose float64 value lies within B (1 + zeta R) 2^-24 cosh(zeta R) of the
threshold (B from the operation count, temporal_gen_ref) are at most 0.1 % of the ordered pairs.

On the GPU: outside the band the edge set is the restatement's, inside either answer is accepted; centres ascend and the neighbours of
a centre ascend; the plan the kernels wrote has the bits of the plan gnnmp_plan_create builds from the device's own edge list; the
inputs come back bit for bit from a poisoned slab at every alignment; reruns are bit-identical."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import temporal_gen_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "gnnmp_hyperbolic_graph_f32"
gpu = pytest.mark.gpu


# ---- without a GPU ---------------------------------------------------------------------------------------------------------------------
def test_header_symbols_and_library_carry_the_export():
    import abi_cases as A
    from gnnmp import _lib
    header = open(os.path.join(ROOT, "include", "gnnmp.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    assert f"int {NAME}(" in header and NAME in _lib.SYMBOLS and NAME in exported
    hdr = A.parse_header()
    decls, _ = hdr
    assert NAME in decls and NAME not in A.must_be_covered(decls, _lib.SYMBOLS, hdr.records)    # a plan handle and the status, nothing else
    import gnnmp
    for f in ("hyperbolic_graph", "rand_temporal_radius_graph", "rand_temporal_hyperbolic_graph"):
        assert callable(getattr(gnnmp, f))


def _call(lib, out=True, points=1, N=4, R=1.0, zeta=1.0, gi=None, ib=8, base=1, G=1):
    P = lambda v: ctypes.c_void_p(0x1000 * v) if v else None     # never dereferenced: the call must refuse first
    h = ctypes.c_void_p(0xdead)
    rc = lib.gnnmp_hyperbolic_graph_f32(ctypes.byref(h) if out else None, P(points), N, ctypes.c_float(R), ctypes.c_float(zeta), P(gi), ib,
                                        base, G, 0, None)
    assert rc == 0 or not out or h.value is None                 # a refused call hands out no plan
    return rc


def test_argument_validation_needs_no_gpu():
    from gnnmp import _lib
    lib = _lib.load()
    EINVAL = _lib.EINVAL
    assert _call(lib, R=-1.0) == EINVAL and b"negative or NaN" in lib.gnnmp_last_error()
    assert _call(lib, R=float("nan")) == EINVAL
    for z in (0.0, -1.0, float("nan"), float("inf")):
        assert _call(lib, zeta=z) == EINVAL and b"zeta" in lib.gnnmp_last_error()
    # what gnnmp_radius_graph_f32 refuses
    assert _call(lib, N=-1) == EINVAL
    assert _call(lib, points=None) == EINVAL
    assert _call(lib, out=False) == EINVAL
    assert _call(lib, gi=1, ib=5) == EINVAL and b"idx_bytes" in lib.gnnmp_last_error()
    assert _call(lib, gi=1, base=-1) == EINVAL and b"index_base" in lib.gnnmp_last_error()
    assert _call(lib, gi=1, G=0) == EINVAL
    assert _call(lib, N=2**31) == _lib.EUNSUPPORTED


def test_python_mirror_refuses_before_the_device():
    import gnnmp
    import torch
    pts = np.zeros((4, 2), np.float32)
    for kw in (dict(R=-1.0), dict(R=float("nan")), dict(R=1.0, zeta=0.0), dict(R=1.0, zeta=float("inf"))):
        with pytest.raises(ValueError):
            gnnmp.hyperbolic_graph(pts, **kw)
    with pytest.raises(AssertionError, match="The number of snapshots must be greater than 1"):
        gnnmp.rand_temporal_hyperbolic_graph(10, 1, 1.0, 4.0, 0.1)
    with pytest.raises(AssertionError, match="α must be greater than 0"):
        gnnmp.rand_temporal_hyperbolic_graph(10, 5, 0.0, 4.0, 0.1)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError):                        # no CPU fallback
            gnnmp.hyperbolic_graph(pts, 1.0)


def test_the_restatement_agrees_with_the_reference_formula_where_that_is_accurate():
    """every pair of random inputs with zeta R <= 4: the same answer to `<= R` as _hyperbolic_distance restated literally, and the same
    distance to 1e-7; d((1, 1), (1, 1)) = 0 and d is symmetric (GNNGraphs/test/generate.jl)"""
    rng = np.random.default_rng(3)
    for zeta in R.ZETAS:
        for zr in (1.0, 4.0):
            Rr = zr / zeta
            pts = R.hyp_points(rng, 40, Rr, alpha=zeta).astype(np.float64)
            v = R.hyp_v(pts, zeta)
            for i in range(40):
                for j in range(40):
                    if i == j or tuple(pts[i]) == tuple(pts[j]):
                        continue
                    lit = R.hyp_distance_literal(pts[i], pts[j], zeta)
                    mine = R.hyp_distance(pts[i], pts[j], zeta)
                    if np.isnan(lit):                            # its acosh argument rounded below 1: the points all but coincide
                        assert mine < 1e-6
                        continue
                    assert abs(lit - mine) <= 1e-7, (zeta, zr, i, j, lit, mine)
                    if abs(lit - Rr) > 1e-7:
                        assert (lit <= Rr) == (v[i, j] <= np.cosh(zeta * Rr)), (zeta, zr, i, j)
    assert R.hyp_distance((1.0, 1.0), (1.0, 1.0), 1.0) == 0.0 == R.hyp_distance_literal((1.0, 1.0), (1.0, 1.0), 1.0)
    a, b = (1.3, 0.4), (2.1, 5.9)
    assert R.hyp_distance(a, b, 1.0) == R.hyp_distance(b, a, 1.0) > 0.0
    adj, _ = R.hyp_adjacency(R.hyp_points(rng, 60, 4.0), 4.0, 1.0)
    assert np.array_equal(adj, adj.T)


@pytest.mark.parametrize("c", R.cases(), ids=repr)
def test_band_condition_of_every_gpu_input(c):
    """asserted on the reference alone, before any device call"""
    adj, band = R.case_adjacency(c)
    assert R.B == 8.0 and R.BAND_CAP == 1e-3
    frac = R.band_fraction(band)
    print(f"{c.name}: {int(adj.sum())} edges, {int(band.sum())} pairs in the band ({frac:.2e} of the ordered pairs)")
    assert frac <= R.BAND_CAP
    if c.name.startswith("seam"):                                # both kinds of pair are there
        near = adj[np.arange(0, 16, 2), np.arange(1, 16, 2)]
        assert near.any() and not near.all()
    elif len(c.points) >= 6:                                     # the duplicate is joined to its twin, whatever R
        assert adj[2, 3] and adj[3, 2] or (c.gi is not None and c.gi[2] != c.gi[3])


# ---- on the GPU ----------------------------------------------------------------------------------------------------------------------------
def _cpu(v):
    return v.cpu().numpy().astype(np.int64)


def _graph_of(c):
    import gnnmp
    import torch
    dt = torch.int64 if c.ib == 8 else torch.int32
    gi = None if c.gi is None else torch.from_numpy(c.gi + c.base).to(dt).cuda()
    return gnnmp.hyperbolic_graph(torch.from_numpy(c.points).cuda(), c.R, c.zeta, gi, self_loops=c.loops, index_base=c.base, idx_dtype=dt)


@gpu
@pytest.mark.parametrize("c", R.cases(), ids=repr)
def test_hyperbolic_graph_against_float64(c):
    import gnnmp
    import torch
    adj, band = R.case_adjacency(c)
    N = len(c.points)
    g = _graph_of(c)
    assert g.num_nodes == N and g.num_graphs == c.n_graphs and g.s.dtype == (torch.int64 if c.ib == 8 else torch.int32)
    s, t = _cpu(g.s) - c.base, _cpu(g.t) - c.base
    assert s.size == 0 or (s.min() >= 0 and s.max() < N and t.min() >= 0 and t.max() < N)
    assert np.all(np.diff(t * N + s) > 0), "centres ascend, the neighbours of a centre ascend, no edge twice"
    got = np.zeros((N, N), bool)
    got[t, s] = True
    wrong = (got != adj) & ~band
    print(f"{c.name}: {g.num_edges} edges, {int((got != adj).sum())} differ inside the band")
    assert not wrong.any(), f"{int(wrong.sum())} pairs outside the band differ, first {np.argwhere(wrong)[:4].tolist()}"
    assert g.w is not None and g.w.dtype == torch.float32 and g.w.numel() == g.num_edges and bool((g.w == 1).all())
    # the plan the kernels wrote = the plan of the device's own edge list
    assert False in g._plans
    built = gnnmp.Plan(g.s, g.t, N, N, c.base, False)
    for a, b, what in zip(g._plans[False].export(), built.export(), ("rowptr", "col", "eid")):
        assert torch.equal(a, b), what
    again = _graph_of(c)
    assert torch.equal(again.s, g.s) and torch.equal(again.t, g.t)


@gpu
def test_single_node_empty_and_non_finite():
    import gnnmp
    import torch
    one = torch.tensor([[0.5, 1.0]], device="cuda")
    assert gnnmp.hyperbolic_graph(one, 1.0).num_edges == 0
    assert gnnmp.hyperbolic_graph(one, 0.0, self_loops=True).num_edges == 1
    assert gnnmp.hyperbolic_graph(torch.zeros((0, 2), device="cuda"), 1.0).num_edges == 0
    # coincident points are joined at R = 0; a NaN or infinite coordinate joins nothing, not even itself
    pts = torch.tensor([[1.5, 0.3], [1.5, 0.3], [float("nan"), 0.0], [1.0, float("inf")], [1.5, 0.3]], device="cuda")
    g = gnnmp.hyperbolic_graph(pts, 0.0, self_loops=True, index_base=0)
    got = set(zip(_cpu(g.s).tolist(), _cpu(g.t).tolist()))
    assert got == {(a, b) for a in (0, 1, 4) for b in (0, 1, 4)}


@gpu
@pytest.mark.parametrize("shift", [0, 4, 8, 16])
def test_memory_contract(shift):
    """`points` and the indicator carved from ONE poisoned slab between guard bands (tests/abi_cases.py): the search writes nothing the
    caller owns — the inputs come back bit for bit and the guards are untouched — at 16-, 8- and 4-byte shifted starts too; the edge
    index read off the plan is the restatement's"""
    import abi_cases as A
    import torch
    from gnnmp import _lib
    lib = _lib.load()
    for c in [k for k in R.cases() if k.name.startswith(("segs-sorted", "5x30-unsorted", "N65"))]:
        adj, band = R.case_adjacency(c)
        assert not band.any()                                    # the expected edge list is exact
        s, t = R.adjacency_coo(adj, c.base)
        N, dt = len(c.points), (np.int64 if c.ib == 8 else np.int32)
        arrs = [A.Arr("points", "in", c.points)]
        if c.gi is not None:
            arrs.append(A.Arr("graph_indicator", "in", (c.gi + c.base).astype(dt)))
        arrs += [A.Arr("out_src", "out", shape=(len(s),), dtype=dt), A.Arr("out_dst", "out", shape=(len(s),), dtype=dt)]
        shifts = {a.name: shift for a in arrs if shift and shift % a.dtype.itemsize == 0}
        slab = A.Slab(arrs, "cuda", shifts)
        h = ctypes.c_void_p()
        rc = lib.gnnmp_hyperbolic_graph_f32(ctypes.byref(h), slab.ptr("points"), N, ctypes.c_float(c.R), ctypes.c_float(c.zeta),
                                            slab.ptr("graph_indicator") if c.gi is not None else None, c.ib, c.base, c.n_graphs,
                                            int(c.loops), None)
        assert rc == 0, lib.gnnmp_last_error()
        try:
            assert slab.check({}, untouched=True) == []
            info = (ctypes.c_int64 * 8)()
            assert lib.gnnmp_plan_info(h, info) == 0 and info[2] == len(s) and info[1] == N
            assert lib.gnnmp_plan_edge_index(h, c.ib, c.base, slab.ptr("out_src"), slab.ptr("out_dst"), None) == 0
            torch.cuda.synchronize()
            problems = slab.check({"out_src": A.E(s.astype(dt), "exact"), "out_dst": A.E(t.astype(dt), "exact")})
            assert problems == [], (c.name, shift, problems)
        finally:
            lib.gnnmp_plan_destroy(h)
