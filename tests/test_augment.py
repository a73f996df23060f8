"""gnnmp_plan_remove_nodes / gnnmp_plan_add_edges (csrc/plan_edit.hip), the parts that need no device: the header declares both calls
with their parameter names and the binding has them, and every refusal comes before any HIP call.  What runs on the device — the
bit-identity with gnnmp_plan_create, the memory contract, the Python mirror — is in tests/test_plan_edit.py."""
import ctypes

import abi_cases as A

PARAMS = {
    "gnnmp_plan_remove_nodes": ["out", "parent", "remove", "idx_bytes", "index_base", "n_remove", "p", "seed", "node_map_out",
                                "node_new_out", "edge_map_out", "total", "stream"],
    "gnnmp_plan_add_edges": ["out", "parent", "s_new", "t_new", "idx_bytes", "index_base", "m", "n_nodes", "seed", "s_new_out",
                             "t_new_out", "stream"],
}
MAX_SLOTS = 4294901760


# ---- no device ----------------------------------------------------------------------------------------------------------------------
def test_header_declares_both_calls_and_the_binding_has_them():
    from gnnmp import _lib
    decls, _ = A.parse_header()
    for name, want in PARAMS.items():
        assert [p[0] for p in decls[name]] == want, name
        assert name in _lib.SYMBOLS
        assert getattr(_lib.load(), name).argtypes is not None
        assert name in A.PREP_TABLE and name not in A.TABLE          # graph prep that synchronises: the memory-contract table, not the recorded one
    assert "total" in A.HOST_PARAMS


class _FakePlan(ctypes.Structure):
    """the head of csrc/common.h's gnnmp_graph: all the refusals read of a plan"""
    _fields_ = [("n_src", ctypes.c_int64), ("n_dst", ctypes.c_int64), ("n_edges", ctypes.c_int64), ("n_total", ctypes.c_int64),
                ("self_loops", ctypes.c_int), ("tail", ctypes.c_char * 1024)]


P_ = lambda v: ctypes.c_void_p(0x1000 * v) if v else None      # never dereferenced: the call must refuse first  # noqa: E731


def test_refusals_come_before_any_hip_call():
    from gnnmp import _lib
    lib = _lib.load()
    EINVAL, EUNSUPPORTED, err = _lib.EINVAL, _lib.EUNSUPPORTED, lib.gnnmp_last_error
    sq, wide = _FakePlan(n_src=5, n_dst=5, n_edges=7, n_total=7), _FakePlan(n_src=5, n_dst=6, n_edges=7, n_total=7)
    one = _FakePlan(n_src=1, n_dst=1, n_edges=0, n_total=0)
    huge = _FakePlan(n_src=5, n_dst=5, n_edges=MAX_SLOTS - 8, n_total=MAX_SLOTS - 3, self_loops=1)
    pl, wd, on, hg = (ctypes.addressof(v) for v in (sq, wide, one, huge))
    tot = (ctypes.c_int64 * 2)()

    def rm(out=True, parent=pl, remove=1, ib=8, base=1, n=3, p=0.0, total=tot):
        h = ctypes.c_void_p()
        return lib.gnnmp_plan_remove_nodes(ctypes.byref(h) if out else None, parent, P_(remove), ib, base, n, p, 7, P_(2), P_(3), P_(4),
                                           total, None)

    def add(out=True, parent=pl, s=1, t=2, ib=8, base=1, m=3, n=5, so=3, to=4):
        h = ctypes.c_void_p()
        return lib.gnnmp_plan_add_edges(ctypes.byref(h) if out else None, parent, P_(s), P_(t), ib, base, m, n, 7, P_(so), P_(to), None)

    for call in (rm, add):
        assert call(out=False) == EINVAL and b"out is NULL" in err()
        assert call(parent=None) == EINVAL and b"parent is NULL" in err()
        assert call(parent=wd) == EINVAL and b"not a square graph" in err()
        assert call(ib=2) == EINVAL and b"idx_bytes" in err()
        assert call(base=2) == EINVAL and b"index_base" in err()
    assert rm(total=None) == EINVAL and b"total is NULL" in err()
    assert rm(n=-1) == EINVAL and b"negative n_remove" in err()
    for p in (-0.1, 1.5, float("nan")):
        assert rm(remove=None, n=0, p=p) == EINVAL and b"outside [0, 1]" in err(), p
    assert rm(p=0.5) == EINVAL and b"p must be 0 in list mode" in err()
    assert rm(remove=None, n=3) == EINVAL and b"without a remove list" in err()
    assert add(m=-1) == EINVAL and b"negative m" in err()
    assert add(n=4) == EINVAL and b"below the parent's" in err()
    assert add(t=None) == EINVAL and b"go together" in err()
    assert add(s=None, t=None, so=None) == EINVAL and b"s_new_out and t_new_out" in err()
    assert add(parent=on, s=None, t=None, n=1) == EINVAL and b"at least 2 nodes" in err()
    assert add(parent=hg, m=3) == EUNSUPPORTED and b"exceed the plan format" in err()
    assert add(m=MAX_SLOTS) == EUNSUPPORTED and b"exceed the plan format" in err()
    assert add(n=2 ** 31 - 1) == EUNSUPPORTED and b"exceed the plan format" in err()
