"""Edge coalescing and compaction without a GPU: the four exports exist in header, SYMBOLS and library; every bad argument is refused
with its status code and a message before any HIP call (from pointers that are never dereferenced); and the numpy restatement the GPU
tests compare against (tests/transforms_ref.py) reproduces the reference's own test items (GNNGraphs/test/transform.jl:104-137, 284-322,
379-417; GNNGraphs/test/query.jl:9-35)."""
import ctypes
import os
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import transforms_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gnnmp_coalesce_edges", "gnnmp_compact_edges", "gnnmp_has_multi_edges", "gnnmp_has_isolated_nodes")


def test_header_symbols_and_library_carry_the_exports():
    import gnnmp
    from gnnmp import _lib
    header = open(os.path.join(ROOT, "include", "gnnmp.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    for name in NAMES:
        assert f"int {name}(" in header
        assert name in _lib.SYMBOLS
        assert name in exported
    for f in ("coalesce_edges", "remove_multi_edges", "to_bidirected", "to_unidirected", "remove_self_loops", "remove_edges",
              "has_multi_edges", "has_isolated_nodes"):
        assert callable(getattr(gnnmp, f))
    assert "Synchronises the stream (graph prep). */\nint gnnmp_coalesce_edges(" in header
    assert "Synchronises the stream (graph prep). */\nint gnnmp_compact_edges(" in header


def test_the_writing_exports_take_a_const_host_record():
    """the table of tests/abi_cases.py owes no case for them (their device outputs travel in a const host struct, like the heterograph
    exports'); tests/test_transforms.py carries their memory-contract checks"""
    import abi_cases as A
    from gnnmp import _lib
    decls, _ = A.parse_header()
    need = A.must_be_covered(decls, _lib.SYMBOLS)
    for name in NAMES:
        assert name in decls and name not in need
    assert [p[0] for p in decls["gnnmp_coalesce_edges"]] == ["job", "total", "stream"]
    assert [p[0] for p in decls["gnnmp_compact_edges"]] == ["job", "total", "stream"]
    assert decls["gnnmp_coalesce_edges"][0][2] and decls["gnnmp_compact_edges"][0][2]          # const
    assert [p[0] for p in decls["gnnmp_has_multi_edges"]][-2:] == ["result", "stream"]
    assert all(c for _, c in A.device_pointer_params("gnnmp_has_multi_edges", decls["gnnmp_has_multi_edges"]))


P = lambda v: ctypes.c_void_p(0x1000 * v) if v else None     # never dereferenced: the call must refuse first


def _coalesce(lib, job=True, total=True, s=1, t=2, ib=8, base=1, E=4, n=5, mode=0, s_out=3, t_out=4, colptr=5, rowval=6):
    from gnnmp import _lib
    j = _lib.CoalesceJob(P(s), P(t), ib, base, E, n, mode, P(s_out), P(t_out), P(colptr), P(rowval))
    tot = ctypes.c_int64(-7)
    rc = lib.gnnmp_coalesce_edges(ctypes.byref(j) if job else None, ctypes.byref(tot) if total else None, None)
    assert not (job and total) or tot.value == 0               # *total is 0 after every refusal (and for E = 0)
    return rc


def _compact(lib, job=True, total=True, s=1, t=2, w=None, ib=8, base=1, E=4, rule=0, remove=None, n_remove=0, p=0.5, seed=1, s_out=3,
             t_out=4, w_out=None, eid_out=5):
    from gnnmp import _lib
    j = _lib.CompactJob(P(s), P(t), P(w), ib, base, E, rule, P(remove), n_remove, p, seed, P(s_out), P(t_out), P(w_out), P(eid_out))
    tot = ctypes.c_int64(-7)
    rc = lib.gnnmp_compact_edges(ctypes.byref(j) if job else None, ctypes.byref(tot) if total else None, None)
    assert not (job and total) or tot.value == 0
    return rc


def test_argument_validation_needs_no_gpu():
    from gnnmp import _lib
    lib = _lib.load()
    EINVAL, EBOUNDS, OK = _lib.EINVAL, _lib.EBOUNDS, _lib.OK
    err = lib.gnnmp_last_error

    assert _coalesce(lib, job=False) == EINVAL and b"null job" in err()
    assert _coalesce(lib, total=False) == EINVAL and b"null total" in err()
    assert _coalesce(lib, ib=3) == EINVAL and b"idx_bytes 3" in err()
    assert _coalesce(lib, base=2) == EINVAL and b"index_base 2" in err()
    assert _coalesce(lib, mode=3) == EINVAL and b"mode 3" in err()
    assert _coalesce(lib, mode=-1) == EINVAL
    assert _coalesce(lib, E=-1) == EINVAL and b"negative" in err()
    assert _coalesce(lib, n=-1) == EINVAL and b"negative" in err()
    for null in ("s", "t", "s_out", "t_out", "colptr", "rowval"):
        assert _coalesce(lib, **{null: None}) == EINVAL and b"null pointer" in err(), null
    assert _coalesce(lib, n=2**32 + 1) == EBOUNDS and b"32 bits" in err()
    assert _coalesce(lib, E=2**32) == EBOUNDS and b"32-bit" in err()
    assert _coalesce(lib, E=2**31, mode=1) == EBOUNDS                       # the mirrored list has 2 E positions
    assert _coalesce(lib, E=2**31 - 1, ib=4) == EBOUNDS and b"4-byte" in err()   # colptr ends at E + 1 = 2^31
    assert _coalesce(lib, E=0) == OK                                           # touches nothing: the pointers are not real
    assert _coalesce(lib, E=0, s=None, t=None, s_out=None, t_out=None, colptr=None, rowval=None) == OK

    assert _compact(lib, job=False) == EINVAL and b"null job" in err()
    assert _compact(lib, total=False) == EINVAL and b"null total" in err()
    assert _compact(lib, ib=5) == EINVAL and b"idx_bytes 5" in err()
    assert _compact(lib, base=-1) == EINVAL and b"index_base" in err()
    assert _compact(lib, rule=3) == EINVAL and b"rule 3" in err()
    assert _compact(lib, E=-2) == EINVAL and b"negative" in err()
    assert _compact(lib, rule=1, remove=6, n_remove=-1) == EINVAL and b"n_remove" in err()
    assert _compact(lib, rule=1, remove=None, n_remove=2) == EINVAL and b"remove" in err()
    for p in (-0.1, 1.5, float("nan")):
        assert _compact(lib, rule=2, p=p) == EINVAL and b"probability" in err()
    assert _compact(lib, w=6) == EINVAL and b"w_out" in err()
    assert _compact(lib, w_out=6) == EINVAL
    for null in ("s", "t", "s_out", "t_out", "eid_out"):
        assert _compact(lib, **{null: None}) == EINVAL and b"null pointer" in err(), null
    assert _compact(lib, E=2**32) == EBOUNDS
    assert _compact(lib, E=2**31 + 1, ib=4) == EBOUNDS and b"4-byte" in err()
    assert _compact(lib, E=0) == OK
    assert _compact(lib, E=0, rule=2, p=1.0) == OK

    res = ctypes.c_int(-7)
    hme = lambda s=1, t=2, ib=8, base=1, E=4, r=True: lib.gnnmp_has_multi_edges(P(s), P(t), ib, base, E, ctypes.byref(res) if r else None, None)
    assert hme(ib=2) == EINVAL and b"idx_bytes" in err()
    assert hme(base=3) == EINVAL and b"index_base" in err()
    assert hme(r=False) == EINVAL and b"null result" in err()
    assert hme(E=-1) == EINVAL and res.value == 0
    assert hme(s=None) == EINVAL and hme(t=None) == EINVAL and b"null pointer" in err()
    assert hme(E=2**32) == EBOUNDS
    res.value = -7
    assert hme(E=0) == OK and res.value == 0
    assert lib.gnnmp_has_isolated_nodes(None, ctypes.byref(res), None) == EINVAL and b"null plan" in err()


def test_python_mirror_refuses_before_the_device():
    import pytest
    import gnnmp
    from gnnmp import transform
    with pytest.raises(ValueError):
        gnnmp.msgpass.aggr_code("prod")
    assert set(transform._MODES) == {"directed", "mirrored", "undirected"}


# ---- the restatement against the reference's own test items --------------------------------------------------------------------------
def test_restatement_to_bidirected_item():
    s, t = [1, 2, 3, 3, 4], [2, 3, 4, 4, 4]
    w = [1.0, 2.0, 3.0, 4.0, 5.0]
    e = [10.0, 20.0, 30.0, 40.0, 50.0]
    r = R.to_bidirected(s, t, 4, w, e)
    assert r.s.tolist() == [1, 2, 2, 3, 3, 4, 4]
    assert r.t.tolist() == [2, 1, 3, 2, 4, 3, 4]
    assert r.w.tolist() == [1, 1, 2, 2, 3.5, 3.5, 5]
    assert r.edata.tolist() == [10.0, 10.0, 20.0, 20.0, 35.0, 35.0, 50.0]
    assert not R.has_multi_edges(r.s, r.t, 4)
    assert sorted(zip(r.s.tolist(), r.t.tolist())) == sorted(zip(r.t.tolist(), r.s.tolist()))      # is_bidirected


def test_restatement_to_unidirected_item():
    s, t = [1, 2, 3, 4, 4], [2, 3, 4, 3, 4]
    w = [1.0, 2.0, 3.0, 4.0, 5.0]
    e = [10.0, 20.0, 30.0, 40.0, 50.0]
    r = R.to_unidirected(s, t, 4, w, e)
    assert r.s.tolist() == [1, 2, 3, 4] and r.t.tolist() == [2, 3, 4, 4]
    assert r.w.tolist() == [1, 2, 3.5, 5] and r.edata.tolist() == [10.0, 20.0, 35.0, 50.0]
    assert not R.has_multi_edges(r.s, r.t, 4)


def test_restatement_undirected_encoding_round_trips():
    n = 9
    s, t = np.meshgrid(np.arange(1, n + 1), np.arange(1, n + 1))
    s, t = s.reshape(-1), t.reshape(-1)
    idx, maxid = R.edge_encoding(s, t, n, directed=False)
    assert idx.min() == 1 and idx.max() == maxid == n * (n + 1) // 2
    s2, t2 = R.edge_decoding(idx, n, directed=False)
    assert np.array_equal(s2, np.minimum(s, t)) and np.array_equal(t2, np.maximum(s, t))
    order = np.argsort(idx, kind="stable")                      # ascending index = lexicographic (lo, hi)
    pairs = list(zip(s2[order].tolist(), t2[order].tolist()))
    assert pairs == sorted(pairs)


def test_restatement_query_items():
    assert R.has_multi_edges([1, 1, 2, 3], [2, 2, 2, 4], 4)
    assert not R.has_multi_edges([1, 2, 2, 3], [2, 1, 2, 4], 4)
    assert R.has_isolated_nodes([1, 2, 3], [2, 3, 2], 3) is False
    assert R.has_isolated_nodes([1, 2, 3], [2, 3, 2], 3, dir="in") is True


def test_restatement_remove_edges_items():
    s, t = np.array([1, 1, 2, 3]), np.array([2, 3, 4, 5])
    w = np.array([0.1, 0.2, 0.3, 0.4], np.float32)
    edata = np.array([ord(c) for c in "abcd"], np.float32)
    s2, t2, _, _, _ = R.remove_edges(s, t, [1])
    assert s2.tolist() == s[1:].tolist() and t2.tolist() == t[1:].tolist()
    s2, t2, w2, e2, kept = R.remove_edges(s, t, [1, 2, 4], w, edata)
    assert (s2.tolist(), t2.tolist(), w2.tolist()) == ([2], [4], [np.float32(0.3)])
    assert e2.tolist() == [ord("c")] and kept.tolist() == [2]
    assert len(R.remove_edges(s, t, [2, 2, 2])[0]) == 3          # a repeated position is harmless


def _rand_simple_graph(n, m, seed):
    rng = np.random.default_rng(seed)
    codes = rng.choice(n * n, size=m, replace=False)
    return codes // n + 1, codes % n + 1


def test_restatement_remove_multi_edges_item():
    s, t = _rand_simple_graph(10, 20, 3)                          # rand_graph(10, 20)
    s1, t1 = np.concatenate([s, s[:5]]), np.concatenate([t, t[:5]])      # add_edges(g, s[1:5], t[1:5])
    E1 = len(s1)
    r = R.remove_multi_edges(s1, t1, 10, aggr="+")
    assert len(r.s) == 20
    assert sorted(zip(r.s.tolist(), r.t.tolist())) == sorted(zip(s.tolist(), t.tolist()))
    edata = {"e1": np.ones((E1, 3), np.float32), "e2": 2 * np.ones(E1, np.float32)}
    r = R.remove_multi_edges(s1, t1, 10, w=3 * np.ones(E1, np.float32), edata=edata)          # default aggregation is +
    assert len(r.s) == 20
    assert sum(bool(np.all(r.edata["e1"][i] == 2)) for i in range(20)) == 5
    assert int(np.sum(r.edata["e2"] == 4)) == 5
    assert int(np.sum(r.w == 6)) == 5
    assert r.seg_len.tolist().count(2) == 5 and r.seg_len.sum() == E1


def test_restatement_remove_self_loops_item():
    s, t = _rand_simple_graph(10, 20, 4)
    keep = s != t                                                 # (rand_graph draws no self loops)
    s, t = s[keep], t[keep]
    E = len(s)
    s1, t1 = np.concatenate([s, np.arange(1, 6)]), np.concatenate([t, np.arange(1, 6)])     # add_edges(g, 1:5, 1:5)
    E1 = E + 5
    edata = {"e1": np.ones((E1, 3), np.float32), "e2": 2 * np.ones(E1, np.float32)}
    s2, t2, w2, e2, kept = R.remove_self_loops(s1, t1, 3 * np.ones(E1, np.float32), edata)
    assert len(s2) == E and np.array_equal(s2, s) and np.array_equal(t2, t)
    assert w2.shape == (E,) and e2["e1"].shape == (E, 3) and e2["e2"].shape == (E,)
    assert kept.tolist() == list(range(E))


def test_restatement_folds_in_sorted_order_in_float32():
    """the order-sensitive item of tests/test_transforms.py: (1e8 + 1) - 1e8 + 1 in float32, left to right, is 1"""
    e = np.array([1e8, 1.0, -1e8, 1.0], np.float32)
    r = R.remove_multi_edges([2, 2, 2, 2], [3, 3, 3, 3], 4, edata=e)
    assert r.edata.tolist() == [1.0] and r.seg_len.tolist() == [4]
    assert float(np.sum(e.astype(np.float64))) == 2.0             # what an exact sum would give
