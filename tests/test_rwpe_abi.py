"""random_walk_pe without a GPU: the export and its internal variant exist in header, SYMBOLS and library; every bad argument is refused
with GNNMP_EINVAL before any HIP call (from pointers that are never dereferenced); the Python mirror refuses bad arguments before the
device; the numpy restatement the GPU tests compare against (tests/rwpe_ref.py) reproduces the reference's own test item
(GNNGraphs/test/transform.jl:431-440) exactly; and every random case of tests/test_rwpe.py is well conditioned: its float32 fold is
within 1e-5 of the float64 model, norm-wise and element by element."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rwpe_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME, INTERNAL = "gnnmp_random_walk_pe_f32", "gnnmp_debug_random_walk_pe_f32"


def test_header_symbols_and_library_carry_the_exports():
    import gnnmp
    from gnnmp import _lib
    header = open(os.path.join(ROOT, "include", "gnnmp.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    for name in (NAME, INTERNAL):
        assert f"int {name}(" in header
        assert name in _lib.SYMBOLS
        assert name in exported
    internal = header.index("GNNMP_INTERNAL")
    assert header.index(f"int {NAME}(") < internal < header.index(f"int {INTERNAL}(")
    assert "int64_t lds_budget_bytes" in header[header.index(f"int {INTERNAL}("):]
    assert "transform.jl:975-990" in header[:internal]
    assert "Synchronises the stream (graph prep). */\nint gnnmp_random_walk_pe_f32(" in header
    assert callable(gnnmp.random_walk_pe)


def test_tile_and_walk_limit_agree_with_the_header():
    import abi_cases as A
    from gnnmp import _lib
    _, defines = A.parse_header()
    assert int(defines["GNNMP_RWPE_TILE"]) == _lib.RWPE_TILE and _lib.RWPE_TILE >= 4
    assert int(defines["GNNMP_RWPE_MAX_WALK"]) == _lib.RWPE_MAX_WALK == 1024


def test_the_export_takes_a_const_host_record():
    """its device output travels in a const host record, like the coalescing exports': the table of tests/abi_cases.py owes no case for
    it, and tests/test_rwpe.py carries its memory-contract checks"""
    import abi_cases as A
    from gnnmp import _lib
    decls, _ = A.parse_header()
    need = A.must_be_covered(decls, _lib.SYMBOLS)
    for name in (NAME, INTERNAL):
        assert name in decls and name not in need
        assert [p[0] for p in decls[name]][:2] == ["plan_t", "job"] and decls[name][1][2]          # const
    assert [p[0] for p in decls[INTERNAL]] == ["plan_t", "job", "lds_budget_bytes", "stream"]
    assert ctypes.sizeof(_lib.RwpeJob) == 48                 # two pointers, int + padding, two int64, a pointer


P = lambda v: ctypes.c_void_p(0x1000 * v) if v else None     # never dereferenced: the call must refuse first


def _call(lib, plan=1, job=True, w=None, gp=None, ib=8, G=1, K=3, out=2, budget=None):
    from gnnmp import _lib
    j = _lib.RwpeJob(P(w), P(gp), ib, G, K, P(out))
    jp = ctypes.byref(j) if job else None
    if budget is None:
        return lib.gnnmp_random_walk_pe_f32(P(plan), jp, None)
    return lib.gnnmp_debug_random_walk_pe_f32(P(plan), jp, budget, None)


def test_argument_validation_needs_no_gpu():
    from gnnmp import _lib
    lib = _lib.load()
    EINVAL = _lib.EINVAL
    err = lib.gnnmp_last_error
    for budget in (None, 0, 4096):                            # the export and its internal variant refuse alike
        assert _call(lib, plan=None, budget=budget) == EINVAL and b"null plan" in err()
        assert _call(lib, job=False, budget=budget) == EINVAL and b"null job" in err()
        assert _call(lib, out=None, budget=budget) == EINVAL and b"null out" in err()
        for K in (0, -1, 1025, 2**40):
            assert _call(lib, K=K, budget=budget) == EINVAL and b"walk_length" in err(), K
        for ib in (0, 2, 3, 16):
            assert _call(lib, ib=ib, budget=budget) == EINVAL and b"idx_bytes" in err(), ib
            assert _call(lib, ib=ib, gp=3, budget=budget) == EINVAL and b"idx_bytes" in err(), ib
        for G in (0, -4):
            assert _call(lib, gp=3, G=G, budget=budget) == EINVAL and b"n_graphs" in err(), G
    assert _call(lib, budget=-1) == EINVAL and b"lds_budget_bytes" in err()


def test_python_mirror_refuses_before_the_device():
    import gnnmp

    class NotAGraph:
        num_nodes = 3

    for bad in (0, -2, 1025):
        with pytest.raises(ValueError):
            gnnmp.random_walk_pe(_host_graph(), bad)
    for bad in (2.0, "3", None, True):
        with pytest.raises(TypeError):
            gnnmp.random_walk_pe(_host_graph(), bad)
    with pytest.raises(TypeError):
        gnnmp.random_walk_pe(NotAGraph(), 3)


def _host_graph():
    """a GNNGraph that never saw the device: the argument checks must come before anything reads it"""
    import gnnmp
    g = object.__new__(gnnmp.GNNGraph)
    g.num_nodes, g.num_edges, g.num_graphs = 3, 4, 1
    return g


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def test_restatement_reproduces_the_reference_item_exactly():
    """s = [1,2,2,3], t = [2,1,3,2], walk_length = 3 -> [0 0 0; 0.5 1 0.5; 0 0 0] (walk_length x nodes)"""
    want = np.array([[0, 0, 0], [0.5, 1, 0.5], [0, 0, 0]], np.float64)
    assert np.array_equal(R.dense64(*R.KNOWN, 3).T, want)
    got = R.fold32(*R.KNOWN, 3)
    assert got.dtype == np.float32 and np.array_equal(got.T, want.astype(np.float32))
    assert np.array_equal(R.KNOWN_ANSWER.T, want)


def test_restatement_scales_by_the_out_degree_of_the_target():
    """RW = A * Diagonal(dinv), dinv from the OUT-degrees.  On the directed case (in- and out-degrees differ) degrees taken from the
    wrong direction give other encodings, by far more than the bar: the case is not blind to that.  The row-scaled matrix
    Diagonal(dinv) * A is NOT such a variant: (A D)^k and (D A)^k have the same diagonal, term by term — a closed walk c -> j1 -> ... -> c
    contributes the product of its edge weights times one dinv per node it visits, whichever side D stands on — so no graph can tell
    the two apart, and the equality is pinned here instead."""
    g, K = R.semantic_cases()["directed"]
    s, t, n, _ = g
    assert np.any(np.bincount(s, minlength=n) != np.bincount(t, minlength=n))
    model = R.dense64(*g, K)
    assert R.deviation(R.dense64(*g, K, in_degree=True), model)[0] > 1000 * R.BAR
    assert np.allclose(R.dense64(*g, K, row_scaled=True), model, rtol=1e-14, atol=0)
    for name, (gg, KK) in R.semantic_cases().items():
        assert np.allclose(R.dense64(*gg, KK, row_scaled=True), R.dense64(*gg, KK), rtol=1e-13, atol=0), name


def test_restatement_edge_semantics():
    c = R.semantic_cases()
    assert np.all(R.dense64(*c["sink"][0], 6)[3] == 0)                               # no way back to a node without out-edges
    assert R.dense64(*c["self_loop"][0], 1)[0, 0] == 0.5                             # A[0, 0] / deg[0]
    assert np.array_equal(R.dense64(*c["one_node_loop"][0], 4), np.ones((1, 4)))
    assert np.array_equal(R.dense64(*c["one_node_bare"][0], 3), np.zeros((1, 3)))
    s, t, n, _ = c["doubled_edge"][0]
    once = R.dense64(s[1:], t[1:], n, None, 6)
    assert R.deviation(R.dense64(s, t, n, None, 6), once)[0] > 1000 * R.BAR          # the copy counts
    assert np.array_equal(R.dense64(s, t, n, None, 6), R.dense64(s[1:], t[1:], n, np.array([2, 1, 1, 1], np.float32), 6))


def test_every_gpu_case_is_well_conditioned():
    """THE CONDITION ON THE INPUTS: for every case tests/test_rwpe.py runs, the float32 fold in edge order is within 1e-5 of the float64
    model norm-wise and element by element, with exact zeros where the model has zeros (weights in [0.5, 1.5]: every term is >= 0)"""
    from gnnmp import _lib
    refs = R.references(_lib.RWPE_TILE)
    assert {"batch", "batch_weighted", "large", "member0", "member6", "directed"} <= set(refs)
    for name, (g, K, d64, f32_) in refs.items():
        assert d64.shape == f32_.shape == (g[2], K), name
        assert g[3] is None or (g[3].min() >= 0.5 and g[3].max() <= 1.5), name
        nw, ew = R.deviation(f32_, d64)
        assert nw <= R.BAR and ew <= R.BAR, (name, nw, ew)
    T = _lib.RWPE_TILE
    assert [m[2] for m in R.batch_members(T)] == [1, 2, T - 1, T, T + 1, 2 * T + 1, 65]
    lg = R.large_graph()
    assert lg[2] == 300 and len(lg[0]) == 1200
