"""The TopKPool exports (csrc/topk.hip, gnnmp_plan_keep_nodes of csrc/plan_edit.hip) at the C ABI.
Without a device: header, SYMBOLS and library carry them; the header's records are the ctypes records field by field; every refusal the
header lists comes before any HIP call (from pointers that are never dereferenced); the cases of tests/topk_cases.py are in the
registry of tests/abi_cases.py.
On the device: the memory contract of tests/test_abi_memory_contract.py over those cases (that file takes its export lists before
tests/topk_cases.py registers, so its three parametrised checks are run here, with the registry's own slab, run_case and verify), and
the capture, replay, new-values and back-to-back check of tests/test_abi_graph_capture.py for the four exports that only launch."""
import ctypes
import os
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_cases as A  # noqa: E402
import topk_cases as T  # noqa: E402  (registers the cases in A.TABLE / A.PREP_TABLE)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = T.LAUNCH_ONLY + (T.KEEP,)


def _table(export):
    return (A.TABLE if export in A.TABLE else A.PREP_TABLE)[export]


def _dry_ctx(variant=0):
    return A.Ctx(int(A.parse_header()[1]["GNNMP_MIN_LONG_ROW"]), variant=variant)


def test_header_symbols_and_library_carry_the_exports():
    import gnnmp
    from gnnmp import _lib
    header = open(os.path.join(ROOT, "include", "gnnmp.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    for name in ALL:
        assert f"int {name}(" in header and name in _lib.SYMBOLS and name in exported, name
        assert header.index(f"int {name}(") < header.index("GNNMP_INTERNAL")
    assert "pool.jl" in " ".join(" ".join(A.header_comments_of(n)) for n in ALL) and header.count("pool.jl:14-27") >= 2
    for name in T.LAUNCH_ONLY:          # launch-only: their comments never speak of a wait or an allocation
        assert not any(A.WAITS_OR_ALLOCATES.search(t) for t in A.header_comments_of(name)), name
    assert all(callable(getattr(gnnmp, n)) for n in ("TopKPool", "topk_index", "topk_pool", "topk_pool_ad"))


def test_the_header_records_are_the_ctypes_records():
    from gnnmp import _lib
    h = A.parse_header()
    decls, defines = h
    assert [p[0] for p in decls[T.SELECT]] == ["job", "N", "stream"] and decls[T.SELECT][0][2]
    assert [p[0] for p in decls[T.KEEP]] == ["out", "parent", "keep", "node_map_out", "node_new_out", "edge_map_out", "total", "stream"]
    assert [p[0] for p in decls[T.SCORE]] == ["x", "p", "y", "N", "C", "stream"]
    assert [f[0] for f in h.records["gnnmp_topk_t"]] == ["score", "graph_ptr", "idx_bytes", "n_graphs", "k", "ratio", "ties", "lds_budget_bytes",
                                                        "keep", "rank"]
    st = A.struct_of("gnnmp_topk_t")
    assert st is _lib.TopkJob and ctypes.sizeof(st) == 72
    assert [(n, getattr(st, n).offset) for n, _ in st._fields_] == [("score", 0), ("graph_ptr", 8), ("idx_bytes", 16), ("n_graphs", 24), ("k", 32),
                                                                    ("ratio", 40), ("ties", 44), ("lds_budget_bytes", 48), ("keep", 56), ("rank", 64)]
    assert dict(st._fields_)["ratio"] is ctypes.c_float
    assert A.struct_of("gnnmp_topk_gate_t") is _lib.TopkGateJob and A.struct_of("gnnmp_topk_gate_grad_t") is _lib.TopkGateGradJob
    assert (int(defines["GNNMP_TOPK_TIES_FIRST"]), int(defines["GNNMP_TOPK_TIES_ALL"])) == (_lib.TOPK_TIES_FIRST, _lib.TOPK_TIES_ALL) == (0, 1)
    assert [int(defines["GNNMP_TOPK_ACT_" + n]) for n in ("SIGMOID", "TANH", "IDENTITY")] == [_lib.TOPK_ACT_SIGMOID, _lib.TOPK_ACT_TANH,
                                                                                              _lib.TOPK_ACT_IDENTITY]
    assert int(defines["GNNMP_TOPK_GRAD_ROWS"]) == _lib.TOPK_GRAD_ROWS == T.R.GRAD_ROWS


def test_the_case_tables_cover_the_exports():
    from gnnmp import _lib
    h = A.parse_header()
    why = {}
    need = A.must_be_covered(h[0], _lib.SYMBOLS, h.records, why)
    assert all(n in need for n in ALL)
    assert why[T.SCORE] == "param" and why[T.KEEP] == "param" and all(why[n] == "record" for n in (T.SELECT, T.GATE, T.GRAD))
    assert all(n in A.TABLE and n not in A.PREP_TABLE and n in A.capturable() for n in T.LAUNCH_ONLY)
    assert T.KEEP in A.PREP_TABLE and T.KEEP not in A.TABLE
    ctx = _dry_ctx()
    for name in ALL:
        cases = _table(name)(ctx)
        assert len({c.sid for c in cases}) == len(cases) and sum("side" in c.tags for c in cases) == 1 and any("align" in c.tags for c in cases)
    sel = [c.args[0].fields for c in A.TABLE[T.SELECT](ctx)]
    assert {f["idx_bytes"] for f in sel if f["graph_ptr"] is not None} == {4, 8} and any(f["graph_ptr"] is None for f in sel)
    assert {f["ties"] for f in sel} == {0, 1} and any(f["k"] == 0 for f in sel) and any(f["rank"] is None for f in sel)
    assert 0 in {f["lds_budget_bytes"] for f in sel} and T.DEV_FROM_12 in {f["lds_budget_bytes"] for f in sel}          # both routes
    assert {c.args[2] for c in A.TABLE[T.GATE](ctx)} == set(T.CS) and {c.args[0].fields["act"] for c in A.TABLE[T.GATE](ctx)} == {0, 1, 2}
    grad = [c.args[0].fields for c in A.TABLE[T.GRAD](ctx)]
    assert any(f["p"] is None for f in grad) and any(f["dp"] is None and f["p"] is not None for f in grad) and any(f["dy"] is None for f in grad)


def test_the_capture_cases_follow_the_variant_rule():
    import test_abi_graph_capture as C
    for name in T.LAUNCH_ONLY:
        (c0,), (c1,) = C._capture_cases(_dry_ctx(0), name), C._capture_cases(_dry_ctx(1), name)
        problems, differ, floats = C._same_call(c0, c1)
        assert not problems and differ and floats, (name, problems)


P_ = lambda v: ctypes.c_void_p(0x1000 * v) if v else None      # never dereferenced: the call must refuse first  # noqa: E731


def test_refusals_come_before_any_hip_call():
    from gnnmp import _lib
    lib = _lib.load()
    EINVAL, EUNSUPPORTED, OK, err = _lib.EINVAL, _lib.EUNSUPPORTED, _lib.OK, lib.gnnmp_last_error

    def select(job=True, score=1, gp=None, ib=8, G=1, k=4, ratio=0.0, ties=0, budget=0, keep=2, rank=None, N=10):
        j = _lib.TopkJob(P_(score), P_(gp), ib, G, k, ratio, ties, budget, P_(keep), P_(rank))
        return lib.gnnmp_topk_select_f32(ctypes.byref(j) if job else None, N, None)

    assert select(job=False) == EINVAL and b"null job" in err()
    assert select(N=-1) == EINVAL and b"negative N" in err()
    assert select(N=2 ** 31 - 1) == EUNSUPPORTED
    for ib in (0, 2, 16):
        assert select(ib=ib) == EINVAL and b"idx_bytes" in err()
    for G in (0, -3):
        assert select(gp=3, G=G) == EINVAL and b"n_graphs" in err()
    assert select(k=-1) == EINVAL and b"k = -1" in err()
    for ratio in (0.0, -0.5, 1.5, float("nan"), float("inf")):
        assert select(k=0, ratio=ratio) == EINVAL and b"ratio" in err(), ratio
    for ties in (-1, 2):
        assert select(ties=ties) == EINVAL and b"ties" in err()
    assert select(budget=-1) == EINVAL and b"lds_budget_bytes" in err()
    assert select(keep=None) == EINVAL and b"null keep" in err()
    assert select(score=None) == EINVAL and b"null score" in err()

    def score(x=1, p=2, y=3, N=5, C=4):
        return lib.gnnmp_topk_score_f32(P_(x), P_(p), P_(y), N, C, None)
    assert score(N=-1) == EINVAL and score(C=0) == EINVAL and score(p=None) == EINVAL and score(x=None) == EINVAL and score(y=None) == EINVAL
    assert score(N=0) == OK                                       # nothing to do: nothing is launched (there is no device here)

    def gate(job=True, x=1, y=2, nm=3, act=0, out=4, n=5, C=4):
        j = _lib.TopkGateJob(P_(x), P_(y), P_(nm), act, P_(out))
        return lib.gnnmp_topk_gate_f32(ctypes.byref(j) if job else None, n, C, None)
    assert gate(job=False) == EINVAL and gate(n=-1) == EINVAL and gate(C=0) == EINVAL
    for act in (-1, 3):
        assert gate(act=act) == EINVAL and b"act" in err()
    assert gate(x=None) == EINVAL and gate(y=None) == EINVAL and gate(nm=None) == EINVAL and gate(out=None) == EINVAL
    assert gate(n=0) == OK

    def grad(job=True, x=1, y=2, p=3, dout=4, nn=5, act=0, dx=6, dy=None, dp=None, part=None, N=5, C=4):
        j = _lib.TopkGateGradJob(P_(x), P_(y), P_(p), P_(dout), P_(nn), act, P_(dx), P_(dy), P_(dp), P_(part))
        return lib.gnnmp_topk_gate_grad_f32(ctypes.byref(j) if job else None, N, C, None)
    assert grad(job=False) == EINVAL and grad(N=-1) == EINVAL and grad(C=0) == EINVAL and grad(act=7) == EINVAL
    assert grad(dp=7, p=None, part=8) == EINVAL and b"dp needs p and part" in err()
    assert grad(dp=7, part=None) == EINVAL and b"dp needs p and part" in err()
    for missing in ("x", "y", "dout", "nn", "dx"):
        assert grad(**{missing: None}) == EINVAL, missing

    h, tot = ctypes.c_void_p(), (ctypes.c_int64 * 2)()
    assert lib.gnnmp_plan_keep_nodes(None, None, None, None, None, None, tot, None) == EINVAL and b"out is NULL" in err()
    assert lib.gnnmp_plan_keep_nodes(ctypes.byref(h), None, None, None, None, None, tot, None) == EINVAL and b"parent is NULL" in err()


# ---- on the device -------------------------------------------------------------------------------------------------------------------
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
@pytest.mark.parametrize("export", ALL)
def test_writes_all_of_its_output_and_nothing_else(lib, ctx, export):
    plans, failures = A.Plans(lib), []
    try:
        for case in _table(export)(ctx):
            rc, slab, host = A.run_case(lib, case, plans)
            problems = A.verify(case, rc, slab, host)
            if problems:
                failures.append(_fail(case, "natural alignment", problems))
    finally:
        plans.close()
    assert not failures, "\n".join(failures)


@pytest.mark.gpu
@pytest.mark.parametrize("export", ALL)
def test_any_element_aligned_pointer(lib, ctx, export):
    """each pointer argument in turn, then all of them together, 16 bytes but not 128, 8 but not 16, 4 only: 4 bytes is all a caller owes"""
    plans, failures, runs = A.Plans(lib), [], 0
    try:
        for case in [c for c in _table(export)(ctx) if "align" in c.tags]:
            for tag, nbytes in A.SHIFTS.items():
                names = [a.name for a in case.arrs if nbytes % a.dtype.itemsize == 0]
                sets = [(f"{n}+{tag}", {n: nbytes}) for n in names] + ([(f"all+{tag}", {n: nbytes for n in names})] if len(names) > 1 else [])
                for what, shifts in sets:
                    rc, slab, host = A.run_case(lib, case, plans, shifts=shifts)
                    problems = A.verify(case, rc, slab, host)          # (no export here documents a refusal for an under-aligned pointer)
                    runs += 1
                    if problems:
                        failures.append(_fail(case, what, problems))
    finally:
        plans.close()
    assert not failures, "\n".join(failures)
    assert runs >= 12


@pytest.mark.gpu
@pytest.mark.parametrize("export", ALL)
def test_on_a_side_stream(lib, ctx, export):
    import torch
    side = torch.cuda.Stream()
    plans = A.Plans(lib)
    try:
        (case,) = [c for c in _table(export)(ctx) if "side" in c.tags]
        rc, slab, host = A.run_case(lib, case, plans, stream=side)
        problems = A.verify(case, rc, slab, host)
    finally:
        plans.close()
    assert not problems, _fail(case, "side stream", problems)


@pytest.mark.gpu
@pytest.mark.parametrize("export", T.LAUNCH_ONLY)
def test_capture_replay_new_values_and_back_to_back(lib, export):
    """recorded into a HIP graph on a side stream and replayed: no host wait, nothing allocated, the eager bits, new values at the same
    addresses, two replays back to back — the helper of tests/test_abi_graph_capture.py, on the side-stream case of each export"""
    import torch
    import test_abi_graph_capture as C
    C._require_working_capture()
    thr = A.plan_threshold(lib, _dry_ctx().hub.E)
    ctxs = A.Ctx(thr, variant=0), A.Ctx(thr, variant=1)
    side, plans, failures = torch.cuda.Stream(), A.Plans(lib), []
    try:
        for c0, c1 in zip(C._capture_cases(ctxs[0], export), C._capture_cases(ctxs[1], export)):
            problems = C._record_and_replay(lib, c0, c1, plans, side)
            if problems:
                failures.append(f"{export}[{c0.sid}]:\n  " + "\n  ".join(problems))
    finally:
        plans.close()
    assert not failures, "\n".join(failures)
