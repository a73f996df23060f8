"""The C ABI's memory contract (include/gnnmp.h: "every pointer is a DEVICE pointer ... the caller allocates inputs AND outputs"), checked
where the value tests are blind: every device array of a call is carved out of ONE poisoned slab with guard bands (tests/abi_cases.py), so

  * an output element a kernel never wrote still carries the poison (torch.empty would have handed back the previous, correct answer),
  * a store past an array, before it, or into a `const` input is seen bit for bit on the host,
  * every pointer can be shifted by whole elements to the alignments a caller is entitled to pass (16 bytes but not 128, 8 but not 16,
    4 only): the call must be right, or refuse with the status the header documents for that argument, leaving everything untouched,
  * the same call works on a side stream, and does not depend on what an earlier call left in the plan's workspace.

The reference is the float64 / exact restatement of each export in the case table (the oracle where it has one).  Bounds are those of the
existing per-kernel tests: bit-equality where they assert it, 1e-5 of the reference's scale elsewhere (1e-12 for the Float64 entry
points), SPLIT_BOUND for the dense core."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_cases as A  # noqa: E402

gpu = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------------------------------------------
# CPU: the table against the header, the coverage condition, the slab itself
# ------------------------------------------------------------------------------------------------------------------------------------
def _dry_ctx():
    _, defines = A.parse_header()
    return A.Ctx(int(defines["GNNMP_MIN_LONG_ROW"]))


def _all_cases(ctx):
    return [c for table in (A.TABLE, A.PREP_TABLE) for build in table.values() for c in build(ctx)]


def test_every_pointer_writing_export_is_covered_or_excluded_with_a_reason():
    from gnnmp import _lib
    hdr = A.parse_header()
    decls, _ = hdr
    assert set(decls) == set(_lib.SYMBOLS), set(decls) ^ set(_lib.SYMBOLS)
    why = {}
    need = A.must_be_covered(decls, _lib.SYMBOLS, hdr.records, why)
    assert len(need) > 112                                  # the parser sees the ABI: 81 exports write through a parameter, 35 through a record
    # an export that takes `const gnnmp_<x>_t *job` writes through the record's non-const fields: a parser that lost the records would
    # file all of them as "writes nothing" again
    assert sum(w == "record" for w in why.values()) >= 30, why
    assert len(A.EXCLUDED_EXTRA) <= 8, "at most eight exports may be excluded beyond the collective"
    assert all(isinstance(r, str) and len(r) > 20 for r in {**A.EXCLUDED, **A.EXCLUDED_EXTRA}.values())
    # covered by a table, or excluded with its reason: no export is waved through by its name (the plan writers and
    # gnnmp_chain_jobs_export synchronise, so they live in PREP_TABLE, which the capture test does not record)
    covered = set(A.TABLE) | set(A.PREP_TABLE)
    missing = [name for name in need if not (name in covered or name in A.EXCLUDED or name in A.EXCLUDED_EXTRA)]
    assert not missing, f"exports without a case and without a reason: {missing}"
    assert not (covered & (set(A.EXCLUDED) | set(A.EXCLUDED_EXTRA)))
    assert not (set(A.TABLE) & set(A.PREP_TABLE))
    assert "gnnmp_plan_slot_gather_f32" in A.TABLE and "gnnmp_graphconv_chain_f32" in A.TABLE
    assert covered <= set(need), covered - set(need)


def test_the_rule_sees_a_write_through_a_record_and_only_that():
    """the rule on a header of its own: a const record with a non-const pointer field is a write, one level down too; a record of
    inputs, a host field and a handle are not"""
    decls = {"f_writes": [("job", True, True, "const gnnmp_w_t *job"), ("stream", False, False, "gnnmp_stream_t stream")],
             "f_nested": [("tab", True, True, "const gnnmp_outer_t *tab"), ("stream", False, False, "gnnmp_stream_t stream")],
             "f_reads": [("job", True, True, "const gnnmp_r_t *job"), ("total", True, False, "int64_t *total"),
                         ("stream", False, False, "gnnmp_stream_t stream")],
             "f_nostream": [("job", True, True, "const gnnmp_w_t *job")]}
    records = {"gnnmp_w_t": [("x", True, True, "const float *x"), ("n", False, False, "int64_t n"), ("y", True, False, "float *y")],
               "gnnmp_r_t": [("x", True, True, "const float *x"), ("plan", True, False, "gnnmp_graph_t *plan"), ("total", True, False, "int64_t *total")],
               "gnnmp_outer_t": [("n", False, False, "int n"), ("rels", True, True, "const gnnmp_w_t *rels")]}
    why = {}
    assert A.must_be_covered(decls, list(decls), records, why) == ["f_writes", "f_nested"]
    assert why == {"f_writes": "record", "f_nested": "record"}
    assert A.writes_of("f_nested", decls["f_nested"], records) == ([], [("gnnmp_w_t", "y")])


def _check_roles(export, decl_fields, values, records, count):
    """one level of a call: the parameters of a declaration, or the fields of a record"""
    assert len(values) == len(decl_fields), (export, len(values), len(decl_fields))
    for (pname, is_ptr, is_const, text), a in zip(decl_fields, values):
        rtype = A.record_of(text, records) if is_ptr else None
        if isinstance(a, A.PtrTab):             # a const host table of const device pointers: every entry an input array, or NULL
            count[0] += sum(v is not None for v in a.items)
            assert re.fullmatch(r"const \w+ \*const \*\w+", text), f"{export}: '{pname}' is {text!r}, the case passes a table of device pointers"
            assert all(v is None or (v.role == "in" and v.field.rstrip("0123456789") == pname) for v in a.items), (export, pname)
        elif isinstance(a, A.HostArr):
            assert is_ptr and is_const and pname in A.HOST_ARRAYS.get(export, ()), f"{export}: '{pname}' is not documented as a host array"
            assert text.startswith({ctypes.c_int64: "const int64_t *", ctypes.c_int: "const int *"}[a.ctype]), (export, pname, text)
        elif isinstance(a, A.Jobs):
            assert "gnnmp_chain_jobs_t" in text, (export, pname)
        elif isinstance(a, A.PlanTab):
            assert re.fullmatch(r"const gnnmp_graph_t \*const \*\w+", text), (export, pname)
        elif isinstance(a, A.NewPlan):
            assert re.fullmatch(r"gnnmp_graph_t \*\*\w+", text), (export, pname)
        elif isinstance(a, A.Made):
            assert re.fullmatch(r"const gnnmp_graph_t \*\w+", text), (export, pname)
        elif isinstance(a, A.Arr):
            count[0] += 1
            assert is_ptr and rtype is None and not A.is_host_param(export, pname), (export, pname)
            assert a.field == pname, f"{export}: array '{a.name}' is passed as '{pname}'"
            assert (a.role == "in") == is_const, f"{export}: '{pname}' is {'const' if is_const else 'non-const'} in the header, the case says '{a.role}'"
        elif isinstance(a, A.Rec) or (isinstance(a, (list, tuple)) and a and isinstance(a[0], A.Rec)):
            for r in ([a] if isinstance(a, A.Rec) else a):
                assert rtype == r.ctype, f"{export}: '{pname}' is {text!r}, the case passes a {r.ctype}"
                assert list(r.fields) == [f[0] for f in records[rtype]], f"{export}: the fields of {rtype} are {[f[0] for f in records[rtype]]}, the case gives {list(r.fields)}"
                _check_roles(export, records[rtype], list(r.fields.values()), records, count)
        elif isinstance(a, A.Pl):
            assert "gnnmp_graph_t" in text, (export, pname)
        elif a is A.STREAM:
            assert "gnnmp_stream_t" in text, (export, pname)
        elif isinstance(a, A.HostOut):
            assert A.is_host_param(export, pname) and not is_const, (export, pname)
        elif a is None:
            assert is_ptr, (export, pname)
        else:
            assert not is_ptr, f"{export}: '{pname}' is a pointer, the case passes {a!r}"


def test_case_roles_agree_with_the_header():
    """const T * is an input; T * is an output, in-out or caller scratch — for a parameter and for a field of a record alike; every call
    has as many arguments as the declaration, every record as many fields as the header's, in its order"""
    from gnnmp import _lib
    hdr = A.parse_header()
    decls, _ = hdr
    lib_sig = {}
    try:
        lib = _lib.load()
        lib_sig = {name: len(getattr(lib, name).argtypes) for name in (*A.TABLE, *A.PREP_TABLE)}
    except (ImportError, OSError):
        pass
    n, nrec = [0], [0]
    for case in _all_cases(_dry_ctx()):
        decl = decls[case.export]
        if lib_sig:
            assert lib_sig[case.export] == len(decl), case.export
        before = n[0]
        _check_roles(case.export, decl, case.args, hdr.records, n)
        if case.then is not None:                             # the second call of a case: the same rules
            _check_roles(case.then[0], decls[case.then[0]], case.then[1], hdr.records, n)
        if any(isinstance(a, A.Rec) for a in case.args):
            nrec[0] += n[0] - before
    assert n[0] > 2000 and nrec[0] > 200


class _AnyHost(dict):
    """the host results of a dry run: whatever the reference expects of them"""

    class _Any:
        def __eq__(self, other):
            return True

    def __getitem__(self, key):
        return self._Any()


class _NoPlans:
    def get(self, p):
        return ctypes.c_void_p(0x1000)


def _bound_into_the_slab(case):
    """bind() on a CPU slab: the call gets as many arguments as the case, a record argument is a pointer the library's argtypes accept,
    and every pointer field of every record points into the array the case names (or is NULL where the case says None)"""
    from gnnmp import _lib
    slab = A.Slab(case.arrs, device="cpu")
    cargs, host = A.bind(case, slab, _NoPlans())
    assert len(cargs) == len(case.args)
    try:
        argtypes = getattr(_lib.load(), case.export).argtypes
    except (ImportError, OSError):
        argtypes = None
    for k, (a, c) in enumerate(zip(case.args, cargs)):
        if not (isinstance(a, A.Rec) or isinstance(a, (list, tuple))):
            continue
        if argtypes:
            argtypes[k].from_param(c)                     # raises where ctypes would refuse the argument
        recs, objs = ([a], [c._obj]) if isinstance(a, A.Rec) else (list(a), list(c._keep_table))
        for rec, st in zip(recs, objs):
            for fname, v in rec.fields.items():
                if isinstance(v, A.Arr):
                    b = v if v.base is None else v.base
                    lo = slab.t.data_ptr() + b.off
                    assert lo <= getattr(st, fname) <= lo + max(b.nbytes, 0), (case.export, case.sid, fname)
                elif v is None:
                    assert not getattr(st, fname), (case.export, case.sid, fname)


def test_every_record_case_has_a_finite_reference_for_every_output():
    """the dry run of the record builders: each case's reference (the float64 / exact restatement of its family's tests/*_ref.py) is
    evaluated without a GPU, names exactly the out / in-out arrays of the slab, and is finite wherever the call owes a finite value
    (the identities of empty max / min rows are the documented exceptions: infinities, never NaN)"""
    n = 0
    for case in _all_cases(_dry_ctx()):
        if not any(isinstance(a, A.Rec) or isinstance(a, (list, tuple)) for a in case.args) or case.status != A.OK:
            continue
        _bound_into_the_slab(case)
        ref = case.ref(_AnyHost())
        owed = {a.name for a in case.arrs if a.role in ("out", "inout")}
        assert set(ref) == owed, (case.export, case.sid, set(ref) ^ owed)
        for name, e in ref.items():
            v = e.value if isinstance(e, A.E) else e
            if v is None:
                assert e.pred is not None, (case.export, case.sid, name)
                continue
            v = np.asarray(v, np.float64)
            if isinstance(e, A.E) and e.rows is not None:
                v = v[e.rows]
            assert not np.isnan(v).any() or case.export.startswith("gnnmp_hetero_"), (case.export, case.sid, name)      # -Inf + Inf of a + fold over empty max and min rows
            n += 1
    assert n > 900


_LP64 = {"int": 4, "float": 4, "int32_t": 4, "uint32_t": 4, "int64_t": 8, "uint64_t": 8, "double": 8}


def test_every_record_of_the_header_has_its_structure():
    """gnnmp/_lib.py must lay every `typedef struct { ... } gnnmp_<x>_t;` out as the C compiler does on LP64: the same field names in
    the same order, every field at the offset its parsed type gives (a pointer 8 bytes, aligned to its size), the same size"""
    records = A.parse_header().records
    assert len(records) >= 36
    for rtype, fields in records.items():
        st = A.struct_of(rtype)
        assert [f[0] for f in st._fields_] == [f[0] for f in fields], rtype
        off, worst = 0, 1
        for fname, is_ptr, is_const, text in fields:
            base = text.replace("const", "").split("*")[0].split()
            size = 8 if is_ptr else _LP64[base[0]]
            if not is_ptr:
                assert len(base) == 2 and base[1] == fname, (rtype, text)
            off = (off + size - 1) // size * size
            assert getattr(st, fname).offset == off and getattr(st, fname).size == size, (rtype, fname, getattr(st, fname).offset, off)
            off += size
            worst = max(worst, size)
        assert ctypes.sizeof(st) == (off + worst - 1) // worst * worst, rtype


def test_the_table_has_the_shapes_the_contract_is_about():
    ctx = _dry_ctx()
    g = ctx.hub
    deg = g.indeg()
    assert deg[0] == 0 and deg[-1] == 0 and deg[g.n // 2] == 0                          # isolated: first, last, interior
    assert sorted(deg[deg >= ctx.thr]) == [ctx.thr, ctx.thr + 1, 5 * ctx.thr]            # at the threshold, just above, a hub over chunks
    by_export = {}
    for c in _all_cases(ctx):
        by_export.setdefault(c.export, []).append(c)
    for export, cs in by_export.items():
        assert len({c.sid for c in cs}) == len(cs), f"{export}: duplicate case ids"
        assert sum("side" in c.tags for c in cs) == 1, f"{export}: exactly one side-stream case"
        assert any("align" in c.tags for c in cs), f"{export}: no alignment case"
        if cs[0].uses_plan and export in A.TABLE:       # (the workspace test runs over TABLE: a PREP_TABLE call computes nothing on a plan)
            assert any("ws" in c.tags for c in cs), f"{export}: no workspace case"
    widths = {int(c.sid.split("_D")[1].split("_")[0]) for c in by_export["gnnmp_propagate_f32"] if c.sid.startswith("hub")}
    assert widths == set(A.DS)


def _toy(shifts=None):
    x = np.arange(24, dtype=np.float32).reshape(6, 4)
    idx = np.array([2, 0, 5], np.int64)
    arrs = [A.Arr("x", "in", x), A.Arr("idx", "in", idx), A.Arr("out", "out", shape=(3, 4))]
    return x, idx, A.Slab(arrs, device="cpu", shifts=shifts)


def _toy_view(slab, name, dtype, count):
    a = slab.arrs[name]
    return slab.t.numpy()[a.off:a.off + count * np.dtype(dtype).itemsize].view(dtype)


@pytest.mark.parametrize("shift", [0, 4, 8, 16])
def test_slab_reports_a_short_write_an_overrun_and_a_written_input(shift):
    """a stand-in "kernel" in numpy on a CPU slab: right, one element short, one element past, and into an input"""
    shifts = {"x": shift, "out": shift, "idx": 8 if shift else 0}
    x, idx, slab = _toy(shifts)
    ref = {"out": A.E(x[idx], "exact")}
    _toy_view(slab, "out", np.float32, 12)[:] = x[idx].reshape(-1)
    assert slab.check(ref) == []
    assert slab.arrs["out"].off % 256 == shift

    x, idx, slab = _toy(shifts)                              # one element short: the last store of the tail is missing
    _toy_view(slab, "out", np.float32, 12)[:11] = x[idx].reshape(-1)[:11]
    p = slab.check(ref)
    assert len(p) == 1 and "1 of 12 element(s) never written, first at element 11" in p[0], p

    x, idx, slab = _toy(shifts)                              # one element past the end: lands in the guard band
    v = _toy_view(slab, "out", np.float32, 13)
    v[:12] = x[idx].reshape(-1)
    v[12] = 7.0
    p = slab.check(ref)
    assert len(p) == 1 and "stray" in p[0] and "0 bytes past the end of array 'out'" in p[0], p

    x, idx, slab = _toy(shifts)                              # one element before the start
    _toy_view(slab, "out", np.float32, 12)[:] = x[idx].reshape(-1)
    slab.t.numpy()[slab.arrs["out"].off - 4:slab.arrs["out"].off].view(np.float32)[0] = 1.0
    p = slab.check(ref)
    assert len(p) == 1 and "before array 'out'" in p[0], p

    x, idx, slab = _toy(shifts)                              # a store into a const input
    _toy_view(slab, "out", np.float32, 12)[:] = x[idx].reshape(-1)
    _toy_view(slab, "x", np.float32, 24)[5] = -1.0
    p = slab.check(ref)
    assert len(p) == 1 and "inside in array 'x' (element 5)" in p[0], p

    x, idx, slab = _toy(shifts)                              # a wrong value is still a wrong value
    _toy_view(slab, "out", np.float32, 12)[:] = x[idx].reshape(-1) + np.float32(1)
    p = slab.check(ref)
    assert len(p) == 1 and "differ from the reference" in p[0], p

    x, idx, slab = _toy(shifts)                              # a refused call must leave everything untouched
    _toy_view(slab, "out", np.float32, 12)[0] = 1.0
    p = slab.check({}, untouched=True)
    assert len(p) == 1 and "error status" in p[0], p

    _rec_toy_reports_its_three_faults(shift)                # the same faults behind a record argument


def _toy_rec(shifts=None):
    """a record of four fields carved from a CPU slab: `x` read, `short`, `past` and `ok` written"""
    x = np.arange(8, dtype=np.float32)
    rec = A.Rec("gnnmp_toy_t", x=A.Arr("x", "in", x), n=8, short=A.Arr("short", "out", shape=(8,)), past=A.Arr("past", "out", shape=(8,)),
                ok=A.Arr("ok", "out", shape=(8,)))
    case = A.Case("toy", "rec", [rec, A.STREAM], None)
    assert [a.name for a in case.arrs] == ["x", "short", "past", "ok"]           # the slab holds what the record points at
    return x, case, A.Slab(case.arrs, device="cpu", shifts=shifts)


def _rec_toy_reports_its_three_faults(shift):
    """the toy wrapped in a Rec: one field written one element short, one written one element past its end, and a store into the `in`
    field — exactly those three problems, so an array that is reached through a record is watched like any other"""
    shifts = {"x": shift, "short": shift, "past": shift, "ok": shift}
    x, case, slab = _toy_rec(shifts)
    ref = {"short": A.E(x, "exact"), "past": A.E(x + 1, "exact"), "ok": A.E(x + 2, "exact")}
    for name, k in (("short", 0), ("past", 1), ("ok", 2)):
        _toy_view(slab, name, np.float32, 8)[:] = x + k
    assert slab.check(ref) == []

    x, case, slab = _toy_rec(shifts)
    _toy_view(slab, "short", np.float32, 8)[:7] = x[:7]
    v = _toy_view(slab, "past", np.float32, 9)
    v[:8] = x + 1
    v[8] = 7.0
    _toy_view(slab, "ok", np.float32, 8)[:] = x + 2
    _toy_view(slab, "x", np.float32, 8)[3] = -1.0
    p = slab.check(ref)
    assert len(p) == 3, p
    assert "stray" in p[0] and "inside in array 'x' (element 3)" in p[0], p
    assert "stray" in p[1] and "0 bytes past the end of array 'past'" in p[1], p
    assert "output 'short': 1 of 8 element(s) never written, first at element 7" in p[2], p


def test_a_view_is_a_pointer_into_its_base_and_owns_no_bytes():
    panel = A.Arr("panel", "inout", np.zeros((5, 12), np.float32))
    z, out = A.Arr("z", "in", base=panel, offset=0), A.Arr("out", "out", base=panel, offset=8)
    case = A.Case("toy", "view", [A.Rec("gnnmp_toy_t", z=z, out=out, ld=12), A.STREAM], None)
    assert [a.name for a in case.arrs] == ["panel"]
    slab = A.Slab(case.arrs, device="cpu", shifts={"panel": 8})
    assert slab.ptr_of(out).value - slab.ptr_of(z).value == 32 and slab.ptr_of(z).value == slab.ptr("panel").value
    with pytest.raises(AssertionError):
        A.Arr("w", "out", base=A.Arr("ro", "in", np.zeros(4, np.float32)))       # nothing is written through an input


def test_slab_pattern_is_a_nan_at_every_element_alignment():
    pat = np.tile(A.PATTERN, 4)
    for off in (0, 4, 8, 12):
        assert np.isnan(pat[off:off + 4].view(np.float32)[0])
    assert np.isnan(pat[:8].view(np.float64)[0]) and np.isnan(pat[8:16].view(np.float64)[0])
    assert all(int(w) % 2 == 1 for w in pat.view(np.uint32))


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import torch
    assert torch.cuda.is_available()
    from gnnmp import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def ctx(lib):
    dry = _dry_ctx()
    thr = A.plan_threshold(lib, dry.hub.E)          # the threshold a plan of the hub graph's size gets: read, not assumed
    return A.Ctx(thr)


def _cases(ctx, export, tag=None):
    cs = list((A.TABLE if export in A.TABLE else A.PREP_TABLE)[export](ctx))
    return [c for c in cs if tag is None or tag in c.tags]


EXPORTS = sorted(A.TABLE)
# the writers that synchronise (plan export / concat / select / edits, the job table's export) have the same memory contract: the three
# tests below run over both tables; the workspace test, the capture test and the lane-group sweep stay on TABLE
WRITERS = EXPORTS + sorted(A.PREP_TABLE)


def _fail(case, what, problems):
    return f"{case.export}[{case.sid}] {what}:\n  " + "\n  ".join(problems)


@gpu
@pytest.mark.parametrize("export", WRITERS)
def test_writes_all_of_its_output_and_nothing_else(lib, ctx, export):
    plans = A.Plans(lib)
    failures = []
    try:
        for case in _cases(ctx, export):
            rc, slab, host = A.run_case(lib, case, plans)
            problems = A.verify(case, rc, slab, host)
            if problems:
                failures.append(_fail(case, "natural alignment", problems))
    finally:
        plans.close()
    assert not failures, "\n".join(failures)


def _shift_sets(case):
    """each pointer argument in turn, then all of them together, at each of the three alignments"""
    for tag, nbytes in A.SHIFTS.items():
        names = [a.name for a in case.arrs if nbytes % a.dtype.itemsize == 0]
        for n in names:
            yield f"{n}+{tag}", {n: nbytes}
        if len(names) > 1:
            yield f"all+{tag}", {n: nbytes for n in names}


@gpu
@pytest.mark.parametrize("export", WRITERS)
def test_any_element_aligned_pointer(lib, ctx, export):
    plans = A.Plans(lib)
    failures = []
    try:
        for case in _cases(ctx, export, "align"):
            for what, shifts in _shift_sets(case):
                rc, slab, host = A.run_case(lib, case, plans, shifts=shifts)
                allowed = {case.align_status[n] for n in shifts if n in case.align_status}
                if rc != case.status and rc in allowed:
                    problems = slab.check({}, untouched=True)          # a documented refusal: nothing may have been written
                else:
                    problems = A.verify(case, rc, slab, host)
                    if rc != case.status:
                        problems = [f"status {rc} ({lib.gnnmp_last_error().decode()}) is not one the header documents for this argument"]
                if problems:
                    failures.append(_fail(case, what, problems))
    finally:
        plans.close()
    assert not failures, "\n".join(failures)


@gpu
@pytest.mark.parametrize("export", WRITERS)
def test_on_a_side_stream(lib, ctx, export):
    import torch
    side = torch.cuda.Stream()
    plans = A.Plans(lib)
    try:
        (case,) = _cases(ctx, export, "side")
        rc, slab, host = A.run_case(lib, case, plans, stream=side)
        problems = A.verify(case, rc, slab, host)
    finally:
        plans.close()
    assert not problems, _fail(case, "side stream", problems)


def _grow_workspace(lib, ctx, plans):
    """wide calls on the hub graph's plans that grow (and dirty) the plan-owned workspace"""
    wide = [("gnnmp_propagate_f32", "hub_D260"), ("gnnmp_propagate_f64", "hub_D260"), ("gnnmp_edge_softmax_f32", "hub_H129"),
            ("gnnmp_propagate_maxmin_grad_f32", "hub_D260"), ("gnnmp_fused_conv_f32", "hub_D128+0"), ("gnnmp_gat_conv_train_f32", "hub_H2_C8"),
            ("gnnmp_gat_conv_stats_f32", "hub_H2_C8"), ("gnnmp_gat_conv_grad_f32", "hub_H2_C8"),
            ("gnnmp_segment_softmax_f32", "K33_D129")]       # on the segment graph's own plan, which the K33 workspace case shares
    for export, prefix in wide:
        (case,) = [c for c in _cases(ctx, export) if c.sid.startswith(prefix)]
        rc, slab, host = A.run_case(lib, case, plans)
        assert rc == case.status, (export, rc)


@gpu
@pytest.mark.parametrize("export", [e for e in EXPORTS if any("gnnmp_graph_t" in p[3] for p in A.parse_header()[0][e])])
def test_result_does_not_depend_on_earlier_calls_on_the_plan(lib, ctx, export):
    used, fresh = A.Plans(lib), A.Plans(lib)
    failures = []
    try:
        _grow_workspace(lib, ctx, used)
        for case in _cases(ctx, export, "ws"):
            rc1, slab1, host1 = A.run_case(lib, case, used)
            rc2, slab2, host2 = A.run_case(lib, case, fresh)
            assert rc1 == rc2 == case.status
            problems = A.verify(case, rc1, slab1, host1)
            a1, a2 = slab1.t.cpu().numpy(), slab2.t.cpu().numpy()
            for a in case.arrs:
                if a.role in ("out", "inout") and not np.array_equal(a1[a.off:a.off + a.nbytes], a2[a.off:a.off + a.nbytes]):
                    problems.append(f"output '{a.name}' on the used plan is not bit-identical to the same call on a fresh plan")
            if problems:
                failures.append(_fail(case, "after wide calls on the plan", problems))
    finally:
        used.close()
        fresh.close()
    assert not failures, "\n".join(failures)


@gpu
def test_chain_on_host_and_device_packed_jobs_is_bit_equal(lib, ctx):
    """the wave-pair kernel on a job table packed by gnnmp_chain_jobs_create and on one packed by gnnmp_chain_jobs_pack: the two packings
    may place a member graph in another job, and a row's arithmetic does not depend on where its tile falls
    (tests/test_graph_chain.py: test_sharded_equals_unsharded_bit_for_bit) — the same operands give the same bits of `out`"""
    cases = {c.sid: c for c in _cases(ctx, "gnnmp_graphconv_chain_f32")}
    # every pair of cases on one operand set runs, in the table's order (a NaN member, then finite values on the same two handles); the
    # bits are owed where no job is set aside: the fp32 redo of a set-aside job covers ALL members of that job, and which members share a
    # job is the packing's choice
    pairs = [(c, cases[sid[:-len("_host")] + "_device"]) for sid, c in cases.items() if sid.startswith("pair_") and sid.endswith("_host")]
    assert len(pairs) >= len(A.CHAIN_PAIR_SIZES) + 2 and sum("_nan_member" in ch.sid for ch, _ in pairs) == 1
    plans = A.Plans(lib)
    failures = []
    try:
        for ch, cd in pairs:
            outs = []
            for c in (ch, cd):
                rc, slab, host = A.run_case(lib, c, plans)
                assert rc == A.OK, (c.sid, rc)
                info = (ctypes.c_int64 * 8)()
                assert lib.gnnmp_chain_jobs_info(plans.jobs(c.args[1]), info) == A.OK and info[0] > 0, f"{c.sid}: the handle has no jobs"
                outs.append(slab.outputs()["out"])
            assert all(np.array_equal(a0.data, a1.data, equal_nan=True) for a0, a1 in zip(ch.arrs, cd.arrs) if a0.data is not None), ch.sid
            if "_nan_member" not in ch.sid and not np.array_equal(outs[0], outs[1]):
                failures.append(f"{ch.sid} / {cd.sid}: `out` differs between the host-packed and the device-packed job table")
    finally:
        plans.close()
    assert not failures, "\n".join(failures)
