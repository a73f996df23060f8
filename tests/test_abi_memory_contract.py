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
    return [c for build in A.TABLE.values() for c in build(ctx)]


def test_every_pointer_writing_export_is_covered_or_excluded_with_a_reason():
    from gnnmp import _lib
    decls, _ = A.parse_header()
    assert set(decls) == set(_lib.SYMBOLS), set(decls) ^ set(_lib.SYMBOLS)
    need = A.must_be_covered(decls, _lib.SYMBOLS)
    assert len(need) > 80                                   # the parser sees the ABI (94 declarations take a stream)
    assert len(A.EXCLUDED_EXTRA) <= 8, "at most eight exports may be excluded beyond the lifecycle calls and the collective"
    assert all(isinstance(r, str) and len(r) > 20 for r in {**A.EXCLUDED, **A.EXCLUDED_EXTRA}.values())
    missing = []
    for name in need:
        lifecycle = name.startswith(A.LIFECYCLE) and name != "gnnmp_plan_slot_gather_f32"
        if not (name in A.TABLE or lifecycle or name in A.EXCLUDED or name in A.EXCLUDED_EXTRA):
            missing.append(name)
    assert not missing, f"exports without a case and without a reason: {missing}"
    assert not (set(A.TABLE) & (set(A.EXCLUDED) | set(A.EXCLUDED_EXTRA)))
    assert "gnnmp_plan_slot_gather_f32" in A.TABLE
    assert set(A.TABLE) <= set(need), set(A.TABLE) - set(need)


def test_case_roles_agree_with_the_header():
    """const T * is an input; T * is an output, in-out or caller scratch — and every call has as many arguments as the declaration"""
    from gnnmp import _lib
    decls, _ = A.parse_header()
    lib_sig = {}
    try:
        lib = _lib.load()
        lib_sig = {name: len(getattr(lib, name).argtypes) for name in A.TABLE}
    except (ImportError, OSError):
        pass
    n = 0
    for case in _all_cases(_dry_ctx()):
        decl = decls[case.export]
        assert len(case.args) == len(decl), (case.export, case.sid, len(case.args), len(decl))
        if lib_sig:
            assert lib_sig[case.export] == len(decl), case.export
        for (pname, is_ptr, is_const, text), a in zip(decl, case.args):
            if isinstance(a, A.Arr):
                n += 1
                assert is_ptr and not A.is_host_param(case.export, pname), (case.export, pname)
                assert a.name == pname, f"{case.export}: array '{a.name}' is passed as parameter '{pname}'"
                assert (a.role == "in") == is_const, f"{case.export}: '{pname}' is {'const' if is_const else 'non-const'} in the header, the case says '{a.role}'"
            elif isinstance(a, A.Pl):
                assert "gnnmp_graph_t" in text, (case.export, pname)
            elif a is A.STREAM:
                assert "gnnmp_stream_t" in text, (case.export, pname)
            elif isinstance(a, A.HostOut):
                assert A.is_host_param(case.export, pname) and not is_const, (case.export, pname)
            elif a is None:
                assert is_ptr, (case.export, pname)
            else:
                assert not is_ptr, f"{case.export}: '{pname}' is a pointer, the case passes {a!r}"
    assert n > 2000


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
        if cs[0].uses_plan:
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
    cs = list(A.TABLE[export](ctx))
    return [c for c in cs if tag is None or tag in c.tags]


EXPORTS = sorted(A.TABLE)


def _fail(case, what, problems):
    return f"{case.export}[{case.sid}] {what}:\n  " + "\n  ".join(problems)


@gpu
@pytest.mark.parametrize("export", EXPORTS)
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
@pytest.mark.parametrize("export", EXPORTS)
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
@pytest.mark.parametrize("export", EXPORTS)
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
