"""knn_graph / radius_graph without a GPU: the two exports exist in header, SYMBOLS and library; every bad argument is refused with its
status code before any HIP call; and the float64 restatement the GPU tests compare against (tests/neighbors_ref.py) reproduces the
reference's own test items (GNNGraphs/test/generate.jl:39-81)."""
import ctypes
import os
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import neighbors_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gnnmp_knn_graph_f32", "gnnmp_radius_graph_f32")


def test_header_symbols_and_library_carry_the_exports():
    from gnnmp import _lib
    header = open(os.path.join(ROOT, "include", "gnnmp.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    for name in NAMES:
        assert f"int {name}(" in header
        assert name in _lib.SYMBOLS
        assert name in exported
    assert callable(__import__("gnnmp").knn_graph) and callable(__import__("gnnmp").radius_graph)


def _knn(lib, out=True, points=1, N=4, d=3, k=2, gi=None, ib=8, base=1, G=1, loops=0):
    P = lambda v: ctypes.c_void_p(0x1000 * v) if v else None     # never dereferenced: the call must refuse first
    h = ctypes.c_void_p(0xdead)
    rc = lib.gnnmp_knn_graph_f32(ctypes.byref(h) if out else None, P(points), N, d, k, P(gi), ib, base, G, loops, None)
    assert rc == 0 or not out or h.value is None                 # a refused call hands out no plan
    return rc


def _radius(lib, out=True, points=1, N=4, d=3, r=1.0, gi=None, ib=8, base=1, G=1):
    P = lambda v: ctypes.c_void_p(0x1000 * v) if v else None
    h = ctypes.c_void_p(0xdead)
    rc = lib.gnnmp_radius_graph_f32(ctypes.byref(h) if out else None, P(points), N, d, ctypes.c_float(r), P(gi), ib, base, G, 0, None)
    assert rc == 0 or not out or h.value is None
    return rc


def test_argument_validation_needs_no_gpu():
    from gnnmp import _lib
    lib = _lib.load()
    EINVAL = _lib.EINVAL
    assert _knn(lib, k=0) == EINVAL and b"k = 0" in lib.gnnmp_last_error()
    assert _knn(lib, k=-3) == EINVAL
    assert _knn(lib, k=1025) == EINVAL and b"1024" in lib.gnnmp_last_error()
    assert _knn(lib, d=0) == EINVAL and b"d = 0" in lib.gnnmp_last_error()
    assert _knn(lib, N=-1) == EINVAL
    assert _knn(lib, points=None) == EINVAL
    assert _knn(lib, out=False) == EINVAL
    assert _knn(lib, gi=1, ib=3) == EINVAL and b"idx_bytes" in lib.gnnmp_last_error()
    assert _knn(lib, gi=1, base=2) == EINVAL and b"index_base" in lib.gnnmp_last_error()
    assert _knn(lib, gi=1, G=0) == EINVAL
    # fewer points than k (+ 1 without self loops): the reference's assertion, known on the host when there is no indicator
    assert _knn(lib, N=2, k=2) == _lib.EBOUNDS
    assert _knn(lib, N=2**31) == _lib.EUNSUPPORTED

    assert _radius(lib, r=-1.0) == EINVAL and b"negative or NaN" in lib.gnnmp_last_error()
    assert _radius(lib, r=float("nan")) == EINVAL
    assert _radius(lib, d=0) == EINVAL
    assert _radius(lib, N=-1) == EINVAL
    assert _radius(lib, points=None) == EINVAL
    assert _radius(lib, out=False) == EINVAL
    assert _radius(lib, gi=1, ib=5) == EINVAL
    assert _radius(lib, gi=1, base=-1) == EINVAL
    assert _radius(lib, gi=1, G=0) == EINVAL


def test_python_mirror_refuses_before_the_device():
    """argument errors of the mirror that need no device: the reference's types (AssertionError for its @asserts)"""
    import pytest
    import torch
    import gnnmp
    if torch.cuda.is_available():
        pytest.skip("covered on the device by tests/test_neighbors.py")
    with pytest.raises(ValueError):
        gnnmp.knn_graph(np.zeros((4, 3), np.float32), 0)
    with pytest.raises(ValueError):
        gnnmp.radius_graph(np.zeros((4, 3), np.float32), -1.0)
    with pytest.raises(RuntimeError):          # no CPU fallback
        gnnmp.knn_graph(np.zeros((4, 3), np.float32), 2)


# ---- the restatement against the reference's own test items (GNNGraphs/test/generate.jl:39-81) ---------------------------------------
def _degrees(s, t, n):
    return np.bincount(s - 1, minlength=n), np.bincount(t - 1, minlength=n)


def test_restatement_knn_items():
    rng = np.random.default_rng(0)
    n, k = 10, 3
    x = rng.random((n, 3)).astype(np.float32)
    s, t = R.knn_coo(R.knn_ref(x, k)[0])
    assert len(s) == n * k                                              # g.num_edges == n * k
    assert np.all(_degrees(s, t, n)[1] == k)                            # degree(g, dir = :in) == fill(k, n)
    assert not np.any(s == t)                                           # has_self_loops(g) == false
    s, t = R.knn_coo(R.knn_ref(x, k, self_loops=True)[0], dir_out=True)
    assert np.all(_degrees(s, t, n)[0] == k)                            # degree(g, dir = :out) == fill(k, n)
    assert np.any(s == t) and np.sum(s == t) == n                       # has_self_loops(g) == true
    gi = np.array([1, 1, 1, 1, 1, 2, 2, 2, 2, 2])
    s, t = R.knn_coo(R.knn_ref(x, k, gi)[0])
    assert len(s) == n * k and np.all(gi[s - 1] == gi[t - 1])           # no edge crosses the graphs
    assert np.all(_degrees(s, t, n)[1] == k)
    # ties go to the lower index, and a duplicated point is a neighbour at distance 0 (not a self loop)
    x = np.array([[0.0], [1.0], [1.0], [2.0]], np.float32)
    nbr, d2 = R.knn_ref(x, 2)
    assert nbr.tolist() == [[1, 2], [2, 0], [1, 0], [1, 2]] and d2[1].tolist() == [0.0, 1.0]


def test_restatement_radius_items():
    rng = np.random.default_rng(1)
    n, r = 10, 0.5
    x = rng.random((n, 3)).astype(np.float32)
    r2 = float(np.float32(r) * np.float32(r))
    lists = R.radius_ref(x, r2)
    s, t, rowptr = R.radius_coo(lists)
    assert not np.any(s == t) and rowptr[-1] == len(s)
    d = np.sqrt(((x[s - 1].astype(np.float64) - x[t - 1]) ** 2).sum(1))
    assert np.all(d <= r + 1e-6)                                        # every edge is within the radius ...
    full = np.sqrt(((x[:, None].astype(np.float64) - x[None]) ** 2).sum(2))
    assert len(s) == int((full <= r).sum()) - n                         # ... and every pair within it is an edge
    s2, t2, _ = R.radius_coo(R.radius_ref(x, r2, self_loops=True), dir_out=True)
    assert np.sum(s2 == t2) == n and len(s2) == len(s) + n
    gi = np.array([1, 1, 1, 1, 1, 2, 2, 2, 2, 2])
    s3, t3, _ = R.radius_coo(R.radius_ref(x, r2, gi))
    assert np.all(gi[s3 - 1] == gi[t3 - 1]) and len(s3) <= len(s)
    for v in lists:
        assert np.all(np.diff(v) > 0)                                   # neighbours ascend
