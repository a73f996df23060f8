"""The GATConv edge-feature training exports (gnnmp_gat_conv_edge_stats_f32 of csrc/gat_fused.hip; gnnmp_gat_conv_edge_grad_f32,
gnnmp_gat_edge_fold_f32 and gnnmp_gat_edge_fold_grad_f32 of csrc/gat_backward.hip) at the C ABI.
Without a device: header, SYMBOLS and library carry them; the header's record is the ctypes record field by field; every refusal the
header lists comes before any HIP call (from pointers that are never dereferenced and plans that are no plans); the cases of
tests/gat_edge_cases.py are in the registry of tests/abi_cases.py, on the graphs their docstring promises, each with a finite float64
reference for every output.
On the device: the memory contract of tests/test_abi_memory_contract.py over those cases (that file takes its export lists before
tests/gat_edge_cases.py registers, so its parametrised checks are run here, with the registry's own slab, run_case and verify) — full
writes and no strays, any element-aligned pointer, a side stream, a plan whose workspace earlier calls grew — and the capture, replay,
new-values and back-to-back check of tests/test_abi_graph_capture.py.  The bound is the registry's: 1e-5 of the float64 restatement."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_cases as A  # noqa: E402
import gat_edge_cases as T  # noqa: E402  (registers the cases in A.TABLE)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = T.LAUNCH_ONLY
FIELDS = ("Wx_src", "Wx_dst", "a", "edge_score", "stats", "dout", "line", "dsd", "dss", "dWx_src", "dWx_dst", "da", "dscore", "negative_slope")


def _dry_ctx(variant=0):
    return A.Ctx(int(A.parse_header()[1]["GNNMP_MIN_LONG_ROW"]), variant=variant)


def test_header_symbols_and_library_carry_the_exports():
    from gnnmp import _lib
    header = open(os.path.join(ROOT, "include", "gnnmp.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    for name in ALL:
        assert f"int {name}(" in header and name in _lib.SYMBOLS and name in exported, name
        assert header.index(f"int {name}(") < header.index("GNNMP_INTERNAL")
        assert not any(A.WAITS_OR_ALLOCATES.search(t) for t in A.header_comments_of(name)), name      # launch-only
        assert any(name in t for t in A.header_comments_of(name)), name                                # a paragraph of its own
    assert "conv.jl:119-121" in " ".join(A.header_comments_of(T.GRAD)) and "conv.jl:112-167" in header[:header.index("GNNMP_INTERNAL")]


def test_the_header_record_is_the_ctypes_record():
    from gnnmp import _lib
    h = A.parse_header()
    decls = h[0]
    assert [p[0] for p in decls[T.GRAD]] == ["plan", "plan_t", "job", "H", "C", "stream"] and decls[T.GRAD][2][2]      # a const record
    assert [p[0] for p in decls[T.STATS]] == ["plan", "Wx_src", "Wx_dst", "a", "edge_score", "negative_slope", "bias", "act", "out", "stats",
                                              "H", "C", "stream"]
    edge = decls["gnnmp_gat_conv_edge_f32"]
    assert [p for p in decls[T.STATS] if p[0] != "stats"] == edge                                    # the forward plus one argument
    assert [p[0] for p in decls[T.FOLD]] == ["a_e", "W_e", "M", "H", "C", "ein", "stream"]
    assert [p[0] for p in decls[T.FOLD_GRAD]] == ["a_e", "W_e", "dM", "dW_e", "da_e", "H", "C", "ein", "stream"]
    assert tuple(f[0] for f in h.records["gnnmp_gat_edge_grad_t"]) == FIELDS
    assert [f[0] for f in h.records["gnnmp_gat_edge_grad_t"] if f[2]] == list(FIELDS[:6])            # the six inputs are const
    st = A.struct_of("gnnmp_gat_edge_grad_t")
    assert st is _lib.GatEdgeGradJob and ctypes.sizeof(st) == 112
    assert [(n, getattr(st, n).offset) for n, _ in st._fields_] == [(n, 8 * k) for k, n in enumerate(FIELDS)]
    assert dict(st._fields_)["negative_slope"] is ctypes.c_float


def test_the_case_tables_cover_the_exports():
    from gnnmp import _lib
    h = A.parse_header()
    why = {}
    need = A.must_be_covered(h[0], _lib.SYMBOLS, h.records, why)
    assert all(n in need for n in ALL)
    assert why[T.GRAD] == "record" and all(why[n] == "param" for n in (T.STATS, T.FOLD, T.FOLD_GRAD))
    assert all(n in A.TABLE and n not in A.PREP_TABLE and n in A.capturable() for n in ALL)
    ctx = _dry_ctx()
    for name in ALL:
        cases = A.TABLE[name](ctx)
        assert len({c.sid for c in cases}) == len(cases) and sum("side" in c.tags for c in cases) == 1 and any("align" in c.tags for c in cases)
        assert not cases[0].uses_plan or any("ws" in c.tags for c in cases)
        assert {c.no_warmup for c in cases} == {False}              # the plans' chunk partials: one eager call comes before a capture
    for name in (T.STATS, T.GRAD):
        cases = A.TABLE[name](ctx)
        hc = {(c.args[-3], c.args[-2]) for c in cases}
        assert hc == {(H, C) for H, C, _ in A.HC}
        refused = [c for c in cases if c.status != A.OK]
        assert [(c.args[-3], c.args[-2], c.status) for c in refused] == [(2, 33, A.EUNSUPPORTED)]
        for H, C, _ in A.HC:                                         # every pair that fits: once with Wx_dst on the bipartite relation, once with NULL
            if T.fits_wave(H, C):
                mine = [c for c in cases if (c.args[-3], c.args[-2]) == (H, C)]
                assert {"ge_sq", "ge_bi"} <= {c.sid.split("_H")[0] for c in mine}
        assert {"ge_sq0", "ge_bi0"} <= {c.sid.split("_H")[0] for c in cases}                           # E = 0
    grad = [c.args[2].fields for c in A.TABLE[T.GRAD](ctx)]
    assert any(f["da"] is None for f in grad) and any(f["da"] is not None for f in grad)
    assert all((f["Wx_dst"] is None) == (f["dWx_dst"] is None) for f in grad) and any(f["Wx_dst"] is not None for f in grad)
    assert all((f["edge_score"] is None) == (f["dscore"] is None) for f in grad) and any(f["dscore"] is None for f in grad)
    fg = A.TABLE[T.FOLD_GRAD](ctx)
    assert any(c.args[3] is None for c in fg) and any(c.args[4] is None for c in fg)


def test_the_graphs_are_the_ones_the_cases_promise():
    ctx = _dry_ctx()
    sq, bi, sq0, bi0 = T.graphs(ctx)
    thr = ctx.thr
    for g in (sq, bi):
        assert (g.n_dst, g.n_src) == (T.N, T.N if g is sq else T.N_SRC_BI)
        deg = g.indeg()
        assert deg[T.ROW9] == 9 and deg[T.ROW70] == 70 and deg[T.ROW_LONG] == T.long_len(thr) > thr
        assert all(deg[i] == 0 for i in T.EMPTY_DST)                                               # rows without in-edges
        short = np.delete(deg, [T.ROW9, T.ROW70, T.ROW_LONG])
        assert short.max() <= thr and abs(int(short.sum()) - 150) <= 1
        out = np.bincount(g.s - 1, minlength=g.n_src)
        assert (out == 0).any() and out.max() > thr and (out[out > 0] <= thr).any()                  # silent sources; plan_t chunks a row, not all
        pairs = (g.s - 1) * T.N + (g.t - 1)
        assert np.bincount(pairs).max() >= 4 and (np.bincount(pairs) >= 2).sum() >= 2              # (s, t) pairs listed several times
        assert g.want_split == int((deg > thr).sum()) >= 1
    assert ((sq.s == T.SELF + 1) & (sq.t == T.SELF + 1)).sum() == 1                                  # an explicit self edge
    assert sq0.E == 0 and bi0.E == 0 and (bi0.n_src, bi0.n_dst) == (T.N_SRC_BI, T.N)
    assert T.graphs(ctx)[0] is sq                                                                  # made once per Ctx: the plans are keyed on it
    sq1 = T.graphs(_dry_ctx(1))[0]
    assert np.array_equal(sq1.s, sq.s) and np.array_equal(sq1.t, sq.t)                               # the same in every variant


def test_every_case_has_a_finite_reference_for_every_output():
    n = 0
    for name in ALL:
        for case in A.TABLE[name](_dry_ctx()):
            if case.status != A.OK:
                continue
            ref = case.ref({})
            assert set(ref) == {a.name for a in case.arrs if a.role in ("out", "inout")}, (name, case.sid)
            for key, e in ref.items():
                v = np.asarray(e.value if isinstance(e, A.E) else e, np.float64)
                if isinstance(e, A.E) and e.rows is not None:
                    v = v[e.rows]
                assert np.isfinite(v).all(), (name, case.sid, key)
                n += 1
    assert n > 80


def test_the_capture_cases_follow_the_variant_rule():
    import test_abi_graph_capture as C
    for name in ALL:
        cs0, cs1 = C._capture_cases(_dry_ctx(0), name), C._capture_cases(_dry_ctx(1), name)
        assert len(cs0) == len(cs1) >= (2 if name in (T.STATS, T.GRAD) else 1)
        for c0, c1 in zip(cs0, cs1):
            problems, differ, floats = C._same_call(c0, c1)
            assert not problems and differ and floats, (name, problems)


P_ = lambda v: ctypes.c_void_p(0x1000 * v) if v else None      # never dereferenced: the call must refuse first  # noqa: E731


class _FakePlan(ctypes.Structure):
    """the head of csrc/common.h's gnnmp_graph {int64 n_src, n_dst, n_edges, n_total; int self_loops; ...}: all the refusals read of a plan"""
    _fields_ = [("n_src", ctypes.c_int64), ("n_dst", ctypes.c_int64), ("n_edges", ctypes.c_int64), ("n_total", ctypes.c_int64),
                ("self_loops", ctypes.c_int), ("tail", ctypes.c_char * 1024)]


def test_refusals_come_before_any_hip_call():
    from gnnmp import _lib
    lib = _lib.load()
    EINVAL, EUNSUPPORTED, OK, err = _lib.EINVAL, _lib.EUNSUPPORTED, _lib.OK, lib.gnnmp_last_error
    fake = lambda ns, nd, e, tot, loops=0: _FakePlan(n_src=ns, n_dst=nd, n_edges=e, n_total=tot, self_loops=loops)      # noqa: E731
    sq, sq_t, loops, tall, bi, bi_t, none = fake(5, 5, 7, 7), fake(5, 5, 7, 7), fake(5, 5, 7, 12, 1), fake(6, 6, 7, 7), fake(3, 5, 7, 7), fake(5, 3, 7, 7), fake(0, 0, 0, 0)
    pl, pt, lp, tl, bp, bt, pn = (ctypes.addressof(v) for v in (sq, sq_t, loops, tall, bi, bi_t, none))

    def grad(plan=pl, plan_t=pt, job=True, Wx_src=1, Wx_dst=None, a=2, es=3, stats=4, dout=5, line=6, dsd=7, dss=8, dWx_src=9, dWx_dst=None, da=10,
             dscore=11, H=2, C=4):
        j = _lib.GatEdgeGradJob(P_(Wx_src), P_(Wx_dst), P_(a), P_(es), P_(stats), P_(dout), line if isinstance(line, ctypes.c_void_p) else P_(line),
                                P_(dsd), P_(dss), P_(dWx_src), P_(dWx_dst), P_(da), P_(dscore), 0.2)
        return lib.gnnmp_gat_conv_edge_grad_f32(plan, plan_t, ctypes.byref(j) if job else None, H, C, None)

    assert grad(plan=None) == EINVAL and b"null plan" in err()
    assert grad(plan_t=None) == EINVAL and b"null plan" in err()
    assert grad(job=False) == EINVAL and b"null job" in err()
    for name in ("Wx_src", "a", "stats", "dout", "line", "dsd", "dss", "dWx_src"):
        assert grad(**{name: None}) == EINVAL and b"null pointer" in err(), name
    assert grad(es=None) == EINVAL and b"null edge_score / dscore" in err()
    assert grad(dscore=None) == EINVAL and b"null edge_score / dscore" in err()
    assert grad(plan=lp, plan_t=lp) == EINVAL and b"self loops" in err() and b"conv.jl:119-121" in err()
    assert grad(plan_t=tl) == EINVAL and b"not the transpose" in err()
    assert grad(line=ctypes.c_void_p(0x6008)) == EINVAL and b"16-byte aligned" in err()
    for H, C in ((0, 4), (2, 0), (-1, 4), (1 << 11, 1 << 11)):
        assert grad(H=H, C=C) == EINVAL and b"bad H/C" in err(), (H, C)
    for H, C in ((65, 4), (1, 130), (5, 13), (2, 33)):                     # 65 lanes of 4, 2 and 1 floats, and abi_cases.HC's wide pair
        assert grad(H=H, C=C) == EUNSUPPORTED and b"fit one wave" in err(), (H, C)
    assert grad(plan=bp, plan_t=bt) == EINVAL and b"bipartite plan needs Wx_dst" in err()
    assert grad(plan=bp, plan_t=bt, Wx_dst=20) == EINVAL and b"needs dWx_dst" in err()
    assert grad(dWx_dst=21) == EINVAL and b"dWx_dst given" in err()
    assert grad(da=None, H=2, C=33) == EUNSUPPORTED                        # (da is nullable: not a refusal of its own)
    assert grad(plan=pn, plan_t=pn, es=None, dscore=None) == OK            # nothing to do: no launch (there is no device here)

    def stats(plan=pl, Wx_src=1, a=2, es=3, out=4, st=5, act=0, H=2, C=4):
        return lib.gnnmp_gat_conv_edge_stats_f32(plan, P_(Wx_src), None, P_(a), P_(es), 0.2, None, act, P_(out), P_(st), H, C, None)
    assert stats(plan=None) == EINVAL
    assert stats(es=None) == EINVAL and b"null edge_score" in err()
    assert stats(plan=lp) == EINVAL and b"add_self_loops" in err()
    assert stats(H=0) == EINVAL and stats(act=2) == EINVAL and stats(out=None) == EINVAL and stats(a=None) == EINVAL
    assert stats(H=2, C=33) == EUNSUPPORTED and b"fits one wave" in err()
    assert stats(plan=bp) == EINVAL and b"bipartite" in err()
    assert stats(plan=pn, es=None) == OK

    def fold(a_e=1, W_e=2, M=3, H=2, C=4, ein=3):
        return lib.gnnmp_gat_edge_fold_f32(P_(a_e), P_(W_e), P_(M), H, C, ein, None)

    def fold_grad(a_e=1, W_e=2, dM=3, dW_e=4, da_e=5, H=2, C=4, ein=3):
        return lib.gnnmp_gat_edge_fold_grad_f32(P_(a_e), P_(W_e), P_(dM), P_(dW_e), P_(da_e), H, C, ein, None)
    for call in (fold, fold_grad):
        for bad in (dict(H=0), dict(C=0), dict(ein=0), dict(H=-2), dict(H=1 << 11, C=1 << 11), dict(ein=(1 << 20) + 1)):
            assert call(**bad) == EINVAL and b"bad H/C/ein" in err(), bad
        assert call(a_e=None) == EINVAL and call(W_e=None) == EINVAL and b"null pointer" in err()
    assert fold(M=None) == EINVAL and fold_grad(dM=None) == EINVAL
    assert fold_grad(dW_e=None, da_e=None) == OK                           # nothing asked for: nothing launched


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
        for case in A.TABLE[export](ctx):
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
    """each pointer argument in turn, then all of them together, 16 bytes but not 128, 8 but not 16, 4 only: the call is right, or refuses
    with the status the header documents for that argument (`line`: GNNMP_EINVAL) and leaves everything untouched"""
    plans, failures, runs, refusals = A.Plans(lib), [], 0, 0
    try:
        for case in [c for c in A.TABLE[export](ctx) if "align" in c.tags]:
            for tag, nbytes in A.SHIFTS.items():
                names = [a.name for a in case.arrs if nbytes % a.dtype.itemsize == 0]
                sets = [(f"{n}+{tag}", {n: nbytes}) for n in names] + ([(f"all+{tag}", {n: nbytes for n in names})] if len(names) > 1 else [])
                for what, shifts in sets:
                    rc, slab, host = A.run_case(lib, case, plans, shifts=shifts)
                    allowed = {case.align_status[n] for n in shifts if n in case.align_status}
                    runs += 1
                    if rc != case.status and rc in allowed:
                        refusals += 1
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
    assert runs >= 12 and (refusals > 0) == (export == T.GRAD)


@pytest.mark.gpu
@pytest.mark.parametrize("export", ALL)
def test_on_a_side_stream(lib, ctx, export):
    import torch
    side = torch.cuda.Stream()
    plans = A.Plans(lib)
    try:
        (case,) = [c for c in A.TABLE[export](ctx) if "side" in c.tags]
        rc, slab, host = A.run_case(lib, case, plans, stream=side)
        problems = A.verify(case, rc, slab, host)
    finally:
        plans.close()
    assert not problems, _fail(case, "side stream", problems)


@pytest.mark.gpu
@pytest.mark.parametrize("export", [T.STATS, T.GRAD])
def test_result_does_not_depend_on_earlier_calls_on_the_plan(lib, ctx, export):
    """the chunk partials live in the plans' workspaces: on plans whose workspace wider calls grew and dirtied, and on fresh ones, the
    same bits — which is also "two calls give equal bits" on the chunked rows of both plans"""
    used, fresh, failures = A.Plans(lib), A.Plans(lib), []
    try:
        for case in [c for c in A.TABLE[export](ctx) if "ws" in c.tags]:
            (wide,) = [c for c in A.TABLE[export](ctx) if c.sid == case.sid.split("_H")[0] + "_H8_C8"]      # 64 floats a row on the same plans
            assert A.run_case(lib, wide, used)[0] == A.OK
            rc1, slab1, host1 = A.run_case(lib, case, used)
            rc2, slab2, host2 = A.run_case(lib, case, fresh)
            assert rc1 == rc2 == case.status
            problems = A.verify(case, rc1, slab1, host1)
            a1, a2 = slab1.t.cpu().numpy(), slab2.t.cpu().numpy()
            for a in case.arrs:
                if a.role in ("out", "inout") and not np.array_equal(a1[a.off:a.off + a.nbytes], a2[a.off:a.off + a.nbytes]):
                    problems.append(f"output '{a.name}' differs between a used and a fresh plan")
            if problems:
                failures.append(_fail(case, "used plan", problems))
    finally:
        used.close()
        fresh.close()
    assert not failures, "\n".join(failures)


@pytest.mark.gpu
@pytest.mark.parametrize("export", ALL)
def test_capture_replay_new_values_and_back_to_back(lib, export):
    """recorded into a HIP graph on a side stream and replayed: no host wait, nothing allocated, the eager bits, new values at the same
    addresses, two replays back to back — the helper of tests/test_abi_graph_capture.py, on the side-stream and workspace cases"""
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
