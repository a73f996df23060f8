"""Heterographs without a GPU: gnnmp_hetero_propagate_f32 exists in header, SYMBOLS and library; every bad argument is refused with its
status before any HIP call; and the restatement the GPU tests compare against (tests/hetero_ref.py) reproduces the reference's own
"Destination node aggregation" test item by hand values (GraphNeuralNetworks/test/layers/heteroconv.jl:39-95, its `+` model)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hetero_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "gnnmp_hetero_propagate_f32"


def test_header_symbols_and_library_carry_the_export():
    import gnnmp
    from gnnmp import _lib
    header = open(os.path.join(ROOT, "include", "gnnmp.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert f"int {NAME}(const gnnmp_hetero_dst_t *dsts, int n_dsts, int64_t D, gnnmp_stream_t stream);" in header
    assert NAME in _lib.SYMBOLS
    assert NAME in {line.split()[-1] for line in nm.splitlines() if line.strip()}
    assert f"#define GNNMP_HETERO_MAX_REL {_lib.HETERO_MAX_REL}\n" in header
    assert _lib.KNOB_HETERO == 22 and "KNOB_HETERO = 22" in open(os.path.join(ROOT, "graphneuralnetworks.jl_amd", "csrc", "common.h")).read()
    for name in ("GNNHeteroGraph", "HeteroGraphConv", "hetero_propagate", "edge_type_subgraph", "rand_heterograph", "rand_bipartite_heterograph",
                 "num_node_types", "num_edge_types"):
        assert hasattr(gnnmp, name), name


def test_the_ctypes_records_have_the_header_layout():
    """gnnmp_hetero_rel_t {plan, x, w, aggr} and gnnmp_hetero_dst_t {out, n_dst, combine, n_rel, rels} as a C compiler lays them out (LP64)"""
    from gnnmp import _lib
    assert ctypes.sizeof(_lib.HeteroRel) == 32 and _lib.HeteroRel.aggr.offset == 24
    assert ctypes.sizeof(_lib.HeteroDst) == 32
    assert [getattr(_lib.HeteroDst, f).offset for f in ("out", "n_dst", "combine", "n_rel", "rels")] == [0, 8, 16, 20, 24]


P = lambda v: ctypes.c_void_p(0x1000 * v) if v else None      # never dereferenced: the call must refuse first  # noqa: E731


def _call(lib, n_dsts=1, D=4, out=1, n_dst=5, combine=0, n_rel=1, rels=True, plan=None, x=2, aggr=0, null_table=False):
    from gnnmp import _lib
    tab = (_lib.HeteroRel * max(n_rel, 1))()
    for r in tab:
        r.plan, r.x, r.w, r.aggr = plan, P(x), None, aggr
    dsts = (_lib.HeteroDst * max(n_dsts, 1))()
    for d in dsts:
        d.out, d.n_dst, d.combine, d.n_rel = P(out), n_dst, combine, n_rel
        d.rels = tab if rels else ctypes.POINTER(_lib.HeteroRel)()
    return lib.gnnmp_hetero_propagate_f32(None if null_table else dsts, n_dsts, D, None)


def test_argument_validation_needs_no_gpu():
    """every refusal comes before the first HIP call: this test runs on a machine without a device, on pointers that are not memory"""
    from gnnmp import _lib
    lib = _lib.load()
    EINVAL, cap = _lib.EINVAL, _lib.HETERO_MAX_REL
    assert _call(lib, null_table=True) == EINVAL and b"destination table" in lib.gnnmp_last_error()
    assert _call(lib, n_dsts=0) == EINVAL
    assert _call(lib, rels=False) == EINVAL and b"relation table" in lib.gnnmp_last_error()
    assert _call(lib, n_rel=0) == EINVAL
    assert _call(lib, D=0) == EINVAL and b"bad D" in lib.gnnmp_last_error()
    assert _call(lib, D=-4) == EINVAL
    assert _call(lib, D=(1 << 20) + 1) == EINVAL
    assert _call(lib, out=None) == EINVAL and b"null out" in lib.gnnmp_last_error()
    assert _call(lib, x=None) == EINVAL and b"null x" in lib.gnnmp_last_error()
    assert _call(lib, n_dst=-1) == EINVAL
    assert _call(lib, n_dst=2**31) == EINVAL
    for bad in (1, 4, -1):                                   # mean is no fold; 4 and -1 are no operator
        assert _call(lib, combine=bad) == EINVAL and b"bad combine" in lib.gnnmp_last_error()
    # more relations than the cap, in one destination type or over several
    assert _call(lib, n_rel=cap + 1) == _lib.EUNSUPPORTED and str(cap).encode() in lib.gnnmp_last_error()
    assert _call(lib, n_dsts=3, n_rel=cap // 2) == _lib.EUNSUPPORTED
    assert _call(lib, n_dsts=cap + 1) == _lib.EUNSUPPORTED


def test_a_call_without_rows_is_accepted_and_launches_nothing():
    """n_dst = 0 everywhere: out may be NULL, no block is launched, the status is OK — on a machine without a device"""
    from gnnmp import _lib
    lib = _lib.load()
    assert _call(lib, n_dst=0, out=None, x=None) == _lib.OK
    assert _call(lib, n_dsts=2, n_dst=0, n_rel=_lib.HETERO_MAX_REL // 2, combine=2, aggr=3) == _lib.OK


def test_a_bad_relation_operator_is_refused_without_a_gpu():
    from gnnmp import _lib
    lib = _lib.load()
    for bad in (4, -1, 17):
        assert _call(lib, aggr=bad) == _lib.EINVAL and b"bad aggr" in lib.gnnmp_last_error()


def test_python_mirror_refuses_before_the_device():
    import torch
    import gnnmp
    with pytest.raises(ValueError):
        gnnmp.HeteroGraphConv({("A", "to", "B"): object()}, aggr="mean")
    with pytest.raises(ValueError):
        gnnmp.HeteroGraphConv([(("A", "to", "B"), object())], aggr="-")
    if torch.cuda.is_available():
        pytest.skip("the graph itself is covered on the device by tests/test_hetero.py")
    with pytest.raises(RuntimeError):          # no CPU fallback
        gnnmp.GNNHeteroGraph({("A", "to", "B"): ([1, 2], [2, 1])})


# ---- the restatement against the reference's own test item (test/layers/heteroconv.jl:39-95) ------------------------------------------
def _reference_item(dtype):
    d, n = 3, 5
    s = np.array([1, 1, 2, 3]) - 1
    t = np.array([1, 2, 2, 3]) - 1
    ets = [("A", "to", "B"), ("B", "to", "A"), ("C", "to", "A")]
    rng = np.random.default_rng(0)
    x = {k: rng.random((n, d)).astype(np.float32) for k in "ABC"}
    ones = np.ones((d, d), np.float32)
    layers = [(et, (ones, ones, None, None, "+")) for et in ets]      # GraphConv(d => d, init = ones, bias = false)
    y = R.hetero_conv_ref(layers, {et: (s, t) for et in ets}, {k: n for k in "ABC"}, x, "+", dtype)
    return x, ones, y


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_restatement_reproduces_the_reference_destination_aggregation_item(dtype):
    x, W, y = _reference_item(dtype)
    col = lambda a, rows: sum(W @ a[r] for r in rows)       # noqa: E731  sum(weights * x[:, rows]; dims = 2)
    # B2 has 2 edges from A and itself
    assert np.allclose(y["B"][1], col(x["A"], [0, 1]) + W @ x["B"][1], rtol=1e-6)
    # B5 has only itself
    assert np.allclose(y["B"][4], W @ x["B"][4], rtol=1e-6)
    # A1 has 1 edge from B, 1 from C and twice itself
    assert np.allclose(y["A"][0], W @ x["B"][0] + W @ x["C"][0] + 2 * (W @ x["A"][0]), rtol=1e-6)
    # A2 has 2 edges from B, 2 from C and twice itself
    assert np.allclose(y["A"][1], col(x["B"], [0, 1]) + col(x["C"], [0, 1]) + 2 * (W @ x["A"][1]), rtol=1e-6)
    # A5 has only itself but twice
    assert np.allclose(y["A"][4], 2 * (W @ x["A"][4]), rtol=1e-6)
    assert list(y) == ["B", "A"] and y["A"].dtype == dtype


def test_restatement_orders_and_identities():
    s, t = np.array([0, 1, 2, 0]), np.array([1, 1, 1, 3])
    x = np.array([[1e8], [1.0], [-1e8]], np.float32)
    # float32, edge order: (1e8 + 1) - 1e8 = 0 in float32, 1 in float64
    assert R.propagate_ref(s, t, 4, x, None, "+", np.float32)[1, 0] == 0.0
    assert R.propagate_ref(s, t, 4, x, None, "+", np.float64)[1, 0] == 1.0
    assert R.propagate_ref(s, t, 4, x, None, "max")[:, 0].tolist() == [-np.inf, 1e8, -np.inf, 1e8]
    assert R.propagate_ref(s, t, 4, x, None, "min")[0, 0] == np.inf
    m = R.propagate_ref(s, t, 4, x, np.array([2, 2, 2, 2], np.float32), "mean")
    assert m[0, 0] == 0.0 and m[3, 0] == 2e8 and m[1, 0] == np.float32(0.0)
    a, b, c = (np.full((1, 1), v, np.float32) for v in (1e8, 1.0, -1e8))
    assert R.fold_ref([a, b, c], "+")[0, 0] == 0.0 and R.fold_ref([a, c, b], "+")[0, 0] == 1.0      # foldl: left to right
    assert R.fold_ref([a, b, c], "max")[0, 0] == 1e8 and R.fold_ref([a, b, c], "min")[0, 0] == -1e8
