"""gnnmp_ppr_diffusion_f32 (csrc/ppr.hip), the parts that need no device: header, SYMBOLS and library carry the export; the header's
record is the ctypes record field by field; every refusal the header lists comes before any HIP call (from pointers that are never
dereferenced and plan heads made on the host); the Python mirror refuses bad arguments by name before the device; the cases of
tests/ppr_cases.py are in the registry of tests/abi_cases.py and pass its dry-run rules.
On the device: the memory contract of tests/test_abi_memory_contract.py over those cases (that file takes its export lists before
tests/ppr_cases.py registers, so its three parametrised checks are run here, with the registry's own slab, run_case and verify), and a
member graph above GNNMP_PPR_MAX_NODES that only graph_ptr reveals."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_cases as A  # noqa: E402
import ppr_cases  # noqa: E402  (registers the export's cases in A.PREP_TABLE)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME, RECORD = "gnnmp_ppr_diffusion_f32", "gnnmp_ppr_t"


def test_header_symbols_and_library_carry_the_export():
    import gnnmp
    from gnnmp import _lib
    header = open(os.path.join(ROOT, "include", "gnnmp.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    assert f"int {NAME}(" in header and NAME in _lib.SYMBOLS and NAME in exported
    assert header.index(f"int {NAME}(") < header.index("GNNMP_INTERNAL")                  # part of the drop-in surface, no debug variant
    assert "transform.jl:1026-1051" in header
    assert f"Synchronises the stream (graph prep). */\nint {NAME}(" in header
    assert "a_ij = fmaf(-f_i, r_j, a_ij)" in header and "UNSPECIFIED" in header
    assert callable(gnnmp.ppr_diffusion)


def test_the_header_record_is_the_ctypes_record():
    from gnnmp import _lib
    h = A.parse_header()
    decls, defines = h
    assert int(defines["GNNMP_PPR_MAX_NODES"]) == _lib.PPR_MAX_NODES == 4096
    assert [p[0] for p in decls[NAME]] == ["plan_t", "job", "stream"] and decls[NAME][1][2]          # a const host record
    fields = h.records[RECORD]
    assert [f[0] for f in fields] == ["w", "graph_ptr", "idx_bytes", "n_graphs", "alpha", "lds_budget_bytes", "out"]
    assert [(f[1], f[2]) for f in fields] == [(True, True), (True, True), (False, False), (False, False), (False, False), (False, False),
                                               (True, False)]
    st = A.struct_of(RECORD)
    assert st is _lib.PprJob
    want = [("w", 0, 8), ("graph_ptr", 8, 8), ("idx_bytes", 16, 4), ("n_graphs", 24, 8), ("alpha", 32, 4), ("lds_budget_bytes", 40, 8),
            ("out", 48, 8)]
    assert [(n, getattr(st, n).offset, getattr(st, n).size) for n, _ in st._fields_] == want
    assert ctypes.sizeof(st) == 56
    assert dict(st._fields_)["alpha"] is ctypes.c_float and dict(st._fields_)["lds_budget_bytes"] is ctypes.c_int64


def _dry_ctx(variant=0):
    return A.Ctx(int(A.parse_header()[1]["GNNMP_MIN_LONG_ROW"]), variant=variant)


def test_the_case_table_covers_the_export():
    from gnnmp import _lib
    h = A.parse_header()
    why = {}
    assert NAME in A.must_be_covered(h[0], _lib.SYMBOLS, h.records, why) and why[NAME] == "record"      # it writes through job->out
    # graph prep that synchronises (its own header comment says so): the memory-contract table, not the recorded one
    assert ppr_cases.NAME == NAME and NAME in A.PREP_TABLE and NAME not in A.TABLE and NAME not in A.EXCLUDED and NAME not in A.EXCLUDED_EXTRA
    assert any("Synchronises the stream (graph prep)" in t for t in A.header_comments_of(NAME))
    cases = A.PREP_TABLE[NAME](_dry_ctx())
    budgets = {c.args[1].fields["lds_budget_bytes"] for c in cases}
    assert 0 in budgets and 160 * 1024 in budgets and any(0 < b < 4 * (12 * 12 + 24) for b in budgets)      # both paths
    assert {c.args[1].fields["idx_bytes"] for c in cases if c.args[1].fields["graph_ptr"] is not None} == {4, 8}
    # the shapes the contract is about, as tests/test_abi_memory_contract.py asks them of every export
    assert len({c.sid for c in cases}) == len(cases) and sum("side" in c.tags for c in cases) == 1 and any("align" in c.tags for c in cases)


def test_the_cases_follow_the_variant_rule():
    """variant 1 of a case is the same call — graph, offsets, budget — on other weights, hence another reference"""
    c0, c1 = A.PREP_TABLE[NAME](_dry_ctx(0)), A.PREP_TABLE[NAME](_dry_ctx(1))
    assert [c.sid for c in c0] == [c.sid for c in c1]
    moved = 0
    for a, b in zip(c0, c1):
        fa, fb = a.args[1].fields, b.args[1].fields
        assert all(fa[k] == fb[k] for k in ("idx_bytes", "n_graphs", "lds_budget_bytes")) and a.args[0].g.name == b.args[0].g.name
        if fa["w"] is not None:
            assert not np.array_equal(fa["w"].data, fb["w"].data)
            moved += 1
    assert moved >= 3


# ---- the memory contract on the device, as tests/test_abi_memory_contract.py checks it for the exports it lists ------------------------------
@pytest.fixture(scope="module")
def lib():
    from gnnmp import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def ctx(lib):
    return A.Ctx(A.plan_threshold(lib, _dry_ctx().hub.E))


def _fail(case, what, problems):
    return f"{case.export}[{case.sid}] {what}:\n  " + "\n  ".join(problems)


@pytest.mark.gpu
def test_writes_all_of_its_output_and_nothing_else(lib, ctx):
    plans, failures = A.Plans(lib), []
    try:
        for case in A.PREP_TABLE[NAME](ctx):
            rc, slab, host = A.run_case(lib, case, plans)
            problems = A.verify(case, rc, slab, host)
            if problems:
                failures.append(_fail(case, "natural alignment", problems))
    finally:
        plans.close()
    assert not failures, "\n".join(failures)


@pytest.mark.gpu
def test_any_element_aligned_pointer(lib, ctx):
    """each pointer argument in turn, then all of them together, 16 bytes but not 128, 8 but not 16, 4 only: 4 bytes is all a caller owes"""
    plans, failures, runs = A.Plans(lib), [], 0
    try:
        for case in [c for c in A.PREP_TABLE[NAME](ctx) if "align" in c.tags]:
            for tag, nbytes in A.SHIFTS.items():
                names = [a.name for a in case.arrs if nbytes % a.dtype.itemsize == 0]
                sets = [(f"{n}+{tag}", {n: nbytes}) for n in names] + ([(f"all+{tag}", {n: nbytes for n in names})] if len(names) > 1 else [])
                for what, shifts in sets:
                    rc, slab, host = A.run_case(lib, case, plans, shifts=shifts)
                    allowed = {case.align_status[n] for n in shifts if n in case.align_status}
                    if rc != case.status and rc in allowed:
                        problems = slab.check({}, untouched=True)          # a documented refusal: nothing may have been written
                    else:
                        problems = A.verify(case, rc, slab, host)
                        if rc != case.status:
                            problems = [f"status {rc} ({lib.gnnmp_last_error().decode()}) is not one the header documents for this argument"]
                    runs += 1
                    if problems:
                        failures.append(_fail(case, what, problems))
    finally:
        plans.close()
    assert not failures, "\n".join(failures)
    assert runs >= 12


@pytest.mark.gpu
def test_on_a_side_stream(lib, ctx):
    import torch
    side = torch.cuda.Stream()
    plans = A.Plans(lib)
    try:
        (case,) = [c for c in A.PREP_TABLE[NAME](ctx) if "side" in c.tags]
        rc, slab, host = A.run_case(lib, case, plans, stream=side)
        problems = A.verify(case, rc, slab, host)
    finally:
        plans.close()
    assert not problems, _fail(case, "side stream", problems)


class _FakePlan(ctypes.Structure):
    """the head of csrc/common.h's gnnmp_graph: all the refusals read of a plan"""
    _fields_ = [("n_src", ctypes.c_int64), ("n_dst", ctypes.c_int64), ("n_edges", ctypes.c_int64), ("n_total", ctypes.c_int64),
                ("self_loops", ctypes.c_int), ("tail", ctypes.c_char * 1024)]


P_ = lambda v: ctypes.c_void_p(0x1000 * v) if v else None      # never dereferenced: the call must refuse first  # noqa: E731


def test_refusals_come_before_any_hip_call():
    from gnnmp import _lib
    lib = _lib.load()
    EINVAL, EUNSUPPORTED, OK, err = _lib.EINVAL, _lib.EUNSUPPORTED, _lib.OK, lib.gnnmp_last_error
    sq = _FakePlan(n_src=5, n_dst=5, n_edges=7, n_total=7)
    loops = _FakePlan(n_src=5, n_dst=5, n_edges=7, n_total=12, self_loops=1)
    wide = _FakePlan(n_src=9, n_dst=5, n_edges=7, n_total=7)
    big = _FakePlan(n_src=4097, n_dst=4097, n_edges=7, n_total=7)
    bare = _FakePlan(n_src=5, n_dst=5, n_edges=0, n_total=0)
    none = _FakePlan(n_src=0, n_dst=0, n_edges=0, n_total=0)
    at = ctypes.addressof

    def call(plan=at(sq), job=True, w=None, gp=None, ib=8, G=1, alpha=0.85, budget=0, out=2):
        j = _lib.PprJob(P_(w), P_(gp), ib, G, alpha, budget, P_(out))
        return lib.gnnmp_ppr_diffusion_f32(plan, ctypes.byref(j) if job else None, None)

    assert call(plan=None) == EINVAL and b"null plan" in err()
    assert call(job=False) == EINVAL and b"null job" in err()
    assert call(out=None) == EINVAL and b"null out" in err()
    for ib in (0, 2, 3, 16):
        assert call(ib=ib) == EINVAL and b"idx_bytes" in err(), ib
        assert call(ib=ib, gp=3) == EINVAL and b"idx_bytes" in err(), ib
    for G in (0, -4):
        assert call(gp=3, G=G) == EINVAL and b"n_graphs" in err(), G
    assert call(plan=at(loops)) == EINVAL and b"added self loops" in err()
    assert call(plan=at(wide)) == EINVAL and b"not square" in err()
    for alpha in (float("nan"), float("inf"), float("-inf")):
        assert call(alpha=alpha) == EINVAL and b"alpha" in err(), alpha
    for budget in (-1, -2 ** 40):
        assert call(budget=budget) == EINVAL and b"lds_budget_bytes" in err(), budget
    # a single graph above the limit is known without the device; the message names the dense need
    assert call(plan=at(big)) == EUNSUPPORTED and b"n x n" in err() and b"4097" in err() and b"GNNMP_PPR_MAX_NODES" in err()
    # nothing to do: no edge (out may be NULL then), no node — GNNMP_OK, and nothing was launched (there is no device here to launch on)
    assert call(plan=at(bare)) == OK and call(plan=at(bare), out=None) == OK and call(plan=at(none), out=None) == OK


def _host_graph():
    """a GNNGraph that never saw the device: the argument checks must come before anything reads it"""
    import gnnmp
    g = object.__new__(gnnmp.GNNGraph)
    g.num_nodes, g.num_edges, g.num_graphs, g.graph_type = 3, 4, 1, "coo"
    return g


def test_python_mirror_refuses_by_name_before_the_device():
    import gnnmp
    from gnnmp.temporal_graph import TemporalSnapshotsGNNGraph

    class NotAGraph:
        num_nodes = 3

    class Hetero:
        is_hetero = True

    for bad in ("0.85", None, 1j, True, [0.85]):
        with pytest.raises(TypeError, match="alpha"):
            gnnmp.ppr_diffusion(_host_graph(), bad)
    for bad in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="not finite"):
            gnnmp.ppr_diffusion(_host_graph(), alpha=bad)
    with pytest.raises(TypeError, match="expected a GNNGraph"):
        gnnmp.ppr_diffusion(NotAGraph())
    with pytest.raises(TypeError, match="GNNHeteroGraph"):
        gnnmp.ppr_diffusion(Hetero())
    with pytest.raises(TypeError, match="TemporalSnapshotsGNNGraph"):
        gnnmp.ppr_diffusion(object.__new__(TemporalSnapshotsGNNGraph))
    sparse = _host_graph()
    sparse.graph_type = "sparse"
    with pytest.raises(TypeError, match="sparse-matrix"):
        gnnmp.ppr_diffusion(sparse)


@pytest.mark.gpu
def test_a_member_above_the_limit_is_unsupported_and_writes_nothing():
    """a fabricated graph_ptr over a small graph: one member of GNNMP_PPR_MAX_NODES + 1 nodes among 8 200 isolated ones.  No n x n block
    is allocated: the sizes are read on the host before anything is."""
    import torch
    from gnnmp import _lib
    lib = _lib.load()
    N = 8200
    s = np.array([1, 2, 3], np.int64)                            # three edges inside the first, small member
    g = A.Graph("ppr_fabricated", s, s[::-1].copy(), N)
    plans = A.Plans(lib)
    try:
        for ib, dt in ((8, np.int64), (4, np.int32)):
            off = np.array([0, 10, 10 + _lib.PPR_MAX_NODES + 1, N], dt)
            slab = A.Slab([A.Arr("graph_ptr", "in", off), A.Arr("out", "out", shape=(3,))])
            job = _lib.PprJob(None, slab.ptr("graph_ptr"), ib, 3, 0.85, 0, slab.ptr("out"))
            rc = lib.gnnmp_ppr_diffusion_f32(plans.get(A.Pl(g, T=True)), ctypes.byref(job), None)
            torch.cuda.synchronize()
            assert rc == _lib.EUNSUPPORTED, (rc, lib.gnnmp_last_error())
            msg = lib.gnnmp_last_error()
            assert b"member graph 1" in msg and b"4097" in msg and b"n x n" in msg
            assert slab.check({}, untouched=True) == []
    finally:
        plans.close()
