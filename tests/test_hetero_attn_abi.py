"""gnnmp_hetero_attn_f32 (csrc/hetero_attn.hip) through the C ABI.

Without a GPU: header, SYMBOLS and the library carry the export; the ctypes records have the header's layout; every refusal of the header
returns its status before any HIP call, on pointers that are not memory and a fake plan head; no instance of the kernel uses scratch
(the code object's notes, as tests/test_tgcn_isa.py reads them); the cases of tests/hetero_attn_cases.py are in the registry of
tests/abi_cases.py, follow its rules and have the row lengths they promise.

On the GPU, every array carved from a poisoned, guarded slab (abi_cases.Slab): every owed element of `out` and of each requested `stats`
written and nothing else, within 1e-5 of the float64 reference (tests/hetero_attn_ref.py) by abi_cases.compare — at every geometry
(one lane .. 64 lanes, odd heads), over empty rows, rows of 1, U - 1, U, U + 1 and G + 1 edges, a row of 300, a relation without edges,
one with a single source, two destination types of different height and one of height 0, GAT and GATv2 mixed, an identity relation
first, all three folds, both activations, bias NULL and given, 16 records; at any element-aligned pointer; on a side stream; recorded
into a HIP graph with no eager call first.  Two calls give equal bits, `out` has the same bits with and without `stats`, and an
R-relation call is bit-identical to folding the R single-relation calls in table order with one fp32 + / max / min each."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_cases as A  # noqa: E402
import hetero_attn_cases as T  # noqa: E402  (registers the cases in A.TABLE)
import hetero_attn_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = T.EXPORT
U = 4      # csrc/hetero_attn.hip: HATTN_U


def _dry_ctx(variant=0):
    return A.Ctx(int(A.parse_header()[1]["GNNMP_MIN_LONG_ROW"]), variant=variant)


# ------------------------------------------------------------------------------------------------------------------------------------
# CPU
# ------------------------------------------------------------------------------------------------------------------------------------
def test_header_symbols_and_library_carry_the_export():
    from gnnmp import _lib
    header = open(os.path.join(ROOT, "include", "gnnmp.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert f"int {NAME}(const gnnmp_hetero_attn_dst_t *dsts, int n_dsts, int64_t H, int64_t C, gnnmp_stream_t stream);" in header
    assert "} gnnmp_hetero_attn_rel_t;" in header and "} gnnmp_hetero_attn_dst_t;" in header
    assert NAME in _lib.SYMBOLS
    assert NAME in {line.split()[-1] for line in nm.splitlines() if line.strip()}
    src = open(os.path.join(ROOT, "graphneuralnetworks.jl_amd", "csrc", "hetero_attn.hip")).read()
    assert "heteroconv.jl:57-86" in src and "conv.jl:112-214" in src and "static_assert" in src and "NOT a measurement" in src


def test_the_ctypes_records_have_the_header_layout():
    """gnnmp_hetero_attn_rel_t {plan, mode, Q, K, a, bias, stats, negative_slope, act} and gnnmp_hetero_attn_dst_t {out, n_dst, combine,
    n_rel, rels} as a C compiler lays them out (LP64), parsed from the header"""
    from gnnmp import _lib
    records = A.parse_header().records
    sizes = {"int": 4, "float": 4, "int64_t": 8}
    for rtype, cls, size in (("gnnmp_hetero_attn_rel_t", _lib.HeteroAttnRel, 64), ("gnnmp_hetero_attn_dst_t", _lib.HeteroAttnDst, 32)):
        assert A.struct_of(rtype) is cls
        assert [f[0] for f in cls._fields_] == [f[0] for f in records[rtype]]
        off = 0
        for fname, is_ptr, _, text in records[rtype]:
            sz = 8 if is_ptr else sizes[text.replace("const", "").split()[0]]
            off = (off + sz - 1) // sz * sz
            assert getattr(cls, fname).offset == off, (rtype, fname)
            off += sz
        assert ctypes.sizeof(cls) == size == (off + 7) // 8 * 8
    assert [getattr(_lib.HeteroAttnRel, f).offset for f in ("plan", "mode", "Q", "K", "a", "bias", "stats", "negative_slope", "act")] == \
        [0, 8, 16, 24, 32, 40, 48, 56, 60]
    assert [getattr(_lib.HeteroAttnDst, f).offset for f in ("out", "n_dst", "combine", "n_rel", "rels")] == [0, 8, 16, 20, 24]


P = lambda v: ctypes.c_void_p(0x1000 * v) if v else None      # never dereferenced: the call must refuse first  # noqa: E731


class _FakePlan(ctypes.Structure):
    """the head of csrc/common.h's gnnmp_graph {int64 n_src, n_dst, n_edges, n_total; int self_loops; ...}: all the refusals read of a
    plan.  The tail is zeroed room for the pointers the call would copy (never dereference) if it did not refuse."""
    _fields_ = [("n_src", ctypes.c_int64), ("n_dst", ctypes.c_int64), ("n_edges", ctypes.c_int64), ("n_total", ctypes.c_int64),
                ("self_loops", ctypes.c_int), ("tail", ctypes.c_char * 1024)]


def _call(lib, n_dsts=1, H=2, C=4, out=1, n_dst=5, combine=0, n_rel=1, rels=True, plan=None, mode=0, Q=2, K=3, a=4, bias=None, stats=None, act=0,
          null_table=False):
    from gnnmp import _lib
    tab = (_lib.HeteroAttnRel * max(n_rel, 1))()
    for r in tab:
        r.plan, r.mode, r.Q, r.K, r.a, r.bias, r.stats, r.negative_slope, r.act = plan, mode, P(Q), P(K), P(a), P(bias), P(stats), 0.2, act
    dsts = (_lib.HeteroAttnDst * max(n_dsts, 1))()
    for d in dsts:
        d.out, d.n_dst, d.combine, d.n_rel = P(out), n_dst, combine, n_rel
        d.rels = tab if rels else ctypes.POINTER(_lib.HeteroAttnRel)()
    return lib.gnnmp_hetero_attn_f32(None if null_table else dsts, n_dsts, H, C, None)


def test_argument_validation_needs_no_gpu():
    """every refusal comes before the first HIP call: this test runs on a machine without a device, on pointers that are not memory"""
    from gnnmp import _lib
    lib = _lib.load()
    EINVAL, EUNS, cap = _lib.EINVAL, _lib.EUNSUPPORTED, _lib.HETERO_MAX_REL
    plan = _FakePlan(n_src=9, n_dst=5, n_edges=7, n_total=7)
    pp = ctypes.addressof(plan)
    err = lambda: lib.gnnmp_last_error()      # noqa: E731
    assert _call(lib, null_table=True) == EINVAL and b"destination table" in err()
    assert _call(lib, n_dsts=0) == EINVAL
    assert _call(lib, rels=False) == EINVAL and b"relation table" in err()
    assert _call(lib, n_rel=0) == EINVAL
    for H, C in ((0, 4), (2, 0), (-1, 4), (2, -3)):
        assert _call(lib, plan=pp, H=H, C=C) == EINVAL and b"bad H/C" in err()
    for combine in (1, 4, -1):      # mean is no fold
        assert _call(lib, plan=pp, combine=combine) == EINVAL and b"bad combine" in err()
    for mode in (2, 3, -1):         # DOT and COS are no members here
        assert _call(lib, plan=pp, mode=mode) == EINVAL and b"bad mode" in err()
    for act in (2, 3, 4, -1):
        assert _call(lib, plan=pp, act=act) == EINVAL and b"bad act" in err()
    assert _call(lib, act=2) == EINVAL                                   # an identity relation's act is checked too
    assert _call(lib, plan=pp, out=None) == EINVAL and b"null out" in err()
    assert _call(lib, plan=pp, Q=None) == EINVAL and b"null Q / a" in err()
    assert _call(lib, plan=pp, a=None) == EINVAL and b"null Q / a" in err()
    assert _call(lib, plan=pp, K=None) == EINVAL and b"null K" in err()
    assert _call(lib, K=None) == EINVAL and b"identity relation" in err()
    assert _call(lib, plan=pp, n_dst=-1) == EINVAL and _call(lib, plan=pp, n_dst=2**31) == EINVAL
    assert _call(lib, plan=pp, n_dst=6) == EINVAL and b"the plan has 5 destinations, the table 6" in err()
    loops = _FakePlan(n_src=5, n_dst=5, n_edges=7, n_total=12, self_loops=1)
    assert _call(lib, plan=ctypes.addressof(loops)) == EINVAL and b"self loops" in err()
    # more records than the cap, in one destination type or over several
    assert _call(lib, plan=pp, n_rel=cap + 1) == EUNS and str(cap).encode() in err()
    assert _call(lib, plan=pp, n_dsts=3, n_rel=cap // 2) == EUNS
    assert _call(lib, n_dsts=cap + 1) == EUNS
    # a feature row that does not fit one wave at the v the pointers allow
    assert _call(lib, plan=pp, H=4, C=65) == EUNS and b"fit one wave" in err()       # v = 1: 260 lanes
    assert _call(lib, plan=pp, H=8, C=64) == EUNS                                     # v = 4: 128 lanes
    # a NULL K is fine on a relation without slots, a NULL everything on a destination type without rows
    empty = _FakePlan(n_src=9, n_dst=0, n_edges=0, n_total=0)
    assert _call(lib, plan=ctypes.addressof(empty), n_dst=0, out=None, Q=None, K=None, a=None) == _lib.OK
    assert _call(lib, plan=ctypes.addressof(empty), H=5, C=20, n_dst=0, out=None, Q=None, K=None, a=None) == _lib.OK      # NULLs admit v = 4: 25 lanes
    assert _call(lib, plan=ctypes.addressof(empty), H=4, C=65, n_dst=0, out=None) == EUNS                                  # refused before "nothing to do"


def test_no_kernel_instance_uses_scratch(tmp_path):
    """the zero-scratch pin of the file header's table: all eight instances hetero_attn_kernel<VEC, 4, LPH> exist in the gfx950 code
    object, none has a private segment or spills, and the widest keeps seven waves a SIMD (at most 72 VGPRs)"""
    import test_tgcn_isa as ISA
    if not (os.path.exists(ISA.OBJDUMP) and os.path.exists(ISA.READELF)):
        pytest.skip("no llvm-objdump / llvm-readelf in this image")
    inst = {}
    for name, notes in ISA.kernel_notes("hetero_attn.o", str(tmp_path)).items():
        m = re.search(r"hetero_attn_kernelILi(\d+)ELi(\d+)ELi(\d+)EE", name)
        if m:
            inst[tuple(int(v) for v in m.groups())] = notes
    assert sorted(inst) == sorted([(4, U, lph) for lph in (0, 1, 2, 4, 8, 16)] + [(2, U, 0), (1, U, 0)]), sorted(inst)
    figures = {}
    for key, n in sorted(inst.items()):
        figures[key] = int(n["vgpr_count"])
        assert int(n["private_segment_fixed_size"]) == 0, f"hetero_attn_kernel{key} uses {n['private_segment_fixed_size']} bytes of scratch"
        assert int(n["vgpr_spill_count"]) == 0 and int(n.get("sgpr_spill_count", 0)) == 0, key
        assert figures[key] <= 72, f"hetero_attn_kernel{key}: {figures[key]} VGPRs, fewer than seven waves a SIMD"
    print("vgpr_count:", figures)


def test_the_cases_are_in_the_registry_and_follow_its_rules():
    from gnnmp import _lib
    hdr = A.parse_header()
    why = {}
    assert NAME in A.must_be_covered(hdr[0], _lib.SYMBOLS, hdr.records, why) and why[NAME] == "record"
    assert NAME not in A.must_be_covered(hdr[0], _lib.SYMBOLS)          # no device pointer among its parameters: const host records
    assert NAME in A.TABLE and NAME not in A.PREP_TABLE and NAME in A.capturable()
    cs0, cs1 = A.TABLE[NAME](_dry_ctx(0)), A.TABLE[NAME](_dry_ctx(1))
    assert len({c.sid for c in cs0}) == len(cs0) == len(T.HC) + 1
    assert sum("side" in c.tags for c in cs0) == 1 and any("align" in c.tags for c in cs0) and any("ws" in c.tags for c in cs0)
    assert all(c.no_warmup and c.uses_plan for c in cs0)
    assert [c.sid for c in cs0] == [c.sid for c in cs1]
    for c0, c1 in zip(cs0, cs1):      # the variants: the same calls on other float inputs
        f0 = [a for a in c0.arrs if a.role == "in"]
        f1 = [a for a in c1.arrs if a.role == "in"]
        assert [(a.name, a.shape) for a in f0] == [(a.name, a.shape) for a in f1]
        assert any(not np.array_equal(a.data, b.data) for a, b in zip(f0, f1))
    n_rec = [sum(r.fields["n_rel"] for r in c.args[0]) for c in cs0]
    assert max(n_rec) == _lib.HETERO_MAX_REL == 16


def test_the_relations_are_the_ones_the_cases_promise():
    G = T.graphs()
    deg = {k: g.indeg() if g.E else np.zeros(g.n_dst, np.int64) for k, g in G.items()}
    into_b = ("main", "one", "none", "rand")
    for i in T.EMPTY_ALL:
        assert all(deg[k][i] == 0 for k in into_b)
    assert deg["main"][12] == 0 and deg["rand"][12] + deg["one"][12] > 0            # empty in one relation only
    assert deg["one"][13] == 0 and deg["main"][13] + deg["rand"][13] > 0
    lengths = set(deg["main"].tolist())
    assert {1, U - 1, U, U + 1, 300} <= lengths and {g + 1 for g in (1, 2, 4, 8, 16, 32, 64)} <= lengths
    assert G["none"].E == 0 and G["one"].n_src == 1 and G["one"].E > 0 and G["to_z"].n_dst == 0
    for H, C in T.HC:                 # n_dst is no multiple of the rows a block takes, at any geometry of the table
        v = 4 if C % 4 == 0 else 2 if C % 2 == 0 else 1
        g = 1
        while g < H * C // v:
            g *= 2
        rows_per_block = (64 // g) * 4
        assert T.NB % rows_per_block != 0 and (g == 1 or T.NB > rows_per_block)
    assert T.NB > 4 * 4 and T.NB % 4 != 0                                            # more than one block at 16 lanes and up
    # every case has a finite reference wherever the call owes a finite value: NaN never, -Inf only as an empty row's maximum
    for c in A.TABLE[NAME](_dry_ctx()):
        ref = c.ref({})
        assert set(ref) == {a.name for a in c.arrs if a.role == "out"}
        for k, e in ref.items():
            v = np.asarray(e.value)
            assert not np.isnan(v).any(), (c.sid, k)
            if k.startswith("out_"):
                assert np.isfinite(v).all(), (c.sid, k)
            else:
                assert np.array_equal(np.isinf(v[..., 0]), v[..., 1] == 0) and np.isfinite(v[..., 1]).all(), (c.sid, k)


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------------------------------------------
gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    import torch
    assert torch.cuda.is_available()
    from gnnmp import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def ctx(lib):
    return A.Ctx(A.plan_threshold(lib, _dry_ctx().hub.E))


def _fail(case, what, problems):
    return f"{case.export}[{case.sid}] {what}:\n  " + "\n  ".join(problems)


def _run(lib, case, plans, shifts=None, stream=None):
    """one call in a fresh slab, verified.  Returns {output name: float32 array}"""
    rc, slab, host = A.run_case(lib, case, plans, shifts=shifts, stream=stream)
    problems = A.verify(case, rc, slab, host)
    assert not problems, _fail(case, "", problems) + f" ({lib.gnnmp_last_error().decode()})"
    after = slab.t.cpu().numpy()
    return {a.name: slab.get(after, a.name).copy() for a in case.arrs if a.role == "out"}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@gpu
def test_writes_all_of_its_output_and_nothing_else(lib, ctx):
    """every geometry, row length and table of the cases, and 16 records in one call"""
    plans, failures = A.Plans(lib), []
    try:
        for case in A.TABLE[NAME](ctx):
            rc, slab, host = A.run_case(lib, case, plans)
            problems = A.verify(case, rc, slab, host)
            if problems:
                failures.append(_fail(case, "natural alignment", problems))
    finally:
        plans.close()
    assert not failures, "\n".join(failures)


@gpu
def test_any_element_aligned_pointer(lib, ctx):
    """each array in turn, then all of them together, 16 bytes but not 128, 8 but not 16, 4 only: the row narrows to v = 2 or 1 and the
    values stay within the bar"""
    plans, failures, runs = A.Plans(lib), [], 0
    try:
        for case in [c for c in A.TABLE[NAME](ctx) if "align" in c.tags]:
            for tag, nbytes in A.SHIFTS.items():
                names = [a.name for a in case.arrs]
                for what, shifts in [(f"{n}+{tag}", {n: nbytes}) for n in names] + [(f"all+{tag}", {n: nbytes for n in names})]:
                    rc, slab, host = A.run_case(lib, case, plans, shifts=shifts)
                    problems = A.verify(case, rc, slab, host)
                    runs += 1
                    if problems:
                        failures.append(_fail(case, what, problems))
    finally:
        plans.close()
    assert not failures, "\n".join(failures)
    assert runs >= 12


@gpu
def test_a_shifted_out_narrows_the_row_or_is_refused(lib):
    """`out` shifted by 4 bytes admits v = 1 only: H*C = 48 is 48 lanes and stays within the bar, H*C = 100 is 100 lanes and refused with
    nothing written; (4, 65) and (8, 64) do not fit at any alignment"""
    G = T.graphs()
    plans = A.Plans(lib)
    dsts = lambda: [("B", T.NB, T.SUM, [T.rel(G["main"], R.GAT, bias=True, stats=True), T.rel(G["rand"], R.GATV2, stats=True, act=1)])]      # noqa: E731
    try:
        _run(lib, T.case("shift48", (), T.draw(dsts(), 4, 12, "shift"), 4, 12), plans, shifts={"out_B": 4})
        _run(lib, T.case("fits100", (), T.draw(dsts(), 5, 20, "shift"), 5, 20), plans)
        for sid, (H, C), shifts in (("shift100", (5, 20), {"out_B": 4}), ("wide260", (4, 65), None), ("wide512", (8, 64), None)):
            case = T.case(sid, (), T.draw(dsts(), H, C, "shift"), H, C, status=-5)
            rc, slab, host = A.run_case(lib, case, plans, shifts=shifts)
            assert rc == -5, (sid, rc)
            assert b"fit one wave" in lib.gnnmp_last_error()
            assert not slab.check({}, untouched=True), sid
    finally:
        plans.close()


@gpu
def test_on_a_side_stream(lib, ctx):
    import torch
    side, plans = torch.cuda.Stream(), A.Plans(lib)
    try:
        (case,) = [c for c in A.TABLE[NAME](ctx) if "side" in c.tags]
        _run(lib, case, plans, stream=side)
    finally:
        plans.close()


@gpu
def test_capture_with_no_eager_call_first_replays_the_eager_bits(lib):
    """recorded into a HIP graph on a side stream and replayed: no host wait, nothing allocated, the eager bits, new values at the same
    addresses, two replays back to back — the helper of tests/test_abi_graph_capture.py, which records a no_warmup case cold"""
    import torch
    import test_abi_graph_capture as C
    C._require_working_capture()
    thr = A.plan_threshold(lib, _dry_ctx().hub.E)
    ctxs = A.Ctx(thr, variant=0), A.Ctx(thr, variant=1)
    side, plans, failures = torch.cuda.Stream(), A.Plans(lib), []
    try:
        pick = lambda cs: [c for c in cs if "side" in c.tags or "ws" in c.tags]      # noqa: E731
        for c0, c1 in zip(pick(A.TABLE[NAME](ctxs[0])), pick(A.TABLE[NAME](ctxs[1]))):
            assert c0.no_warmup
            problems = C._record_and_replay(lib, c0, c1, plans, side)
            if problems:
                failures.append(f"{NAME}[{c0.sid}]:\n  " + "\n  ".join(problems))
    finally:
        plans.close()
    assert not failures, "\n".join(failures)


def _fold32(terms, combine):
    """foldl in float32, one + / max / min each, as Base.max / Base.min order them: a NaN stays, -0.0 < +0.0"""
    out = terms[0].copy()
    for t in terms[1:]:
        if combine == T.SUM:
            out = (out + t).astype(np.float32)
            continue
        pick = (np.maximum(out, t) if combine == T.MAX else np.minimum(out, t)).astype(np.float32)      # numpy propagates NaN, as Julia does
        zeros = (out == 0) & (t == 0)
        neg = (np.signbit(out) & np.signbit(t)) if combine == T.MAX else (np.signbit(out) | np.signbit(t))
        out = np.where(zeros, np.where(neg, np.float32(-0.0), np.float32(0.0)), pick).astype(np.float32)
    return out


@gpu
@pytest.mark.parametrize("H,C", [(2, 3), (4, 8), (4, 64)])
@pytest.mark.parametrize("combine", [T.SUM, T.MAX, T.MIN])
def test_equal_bits_stats_or_not_and_the_fold_of_single_relation_calls(lib, H, C, combine):
    """two calls give equal bits; `out` has the same bits with and without `stats`; the R-relation call is bit-identical (NaN-aware) to
    the R single-relation calls of the same export folded in table order in fp32"""
    G = T.graphs()
    rels = [T.rel(None), T.rel(G["main"], R.GAT, bias=True, stats=True, act=1), T.rel(G["one"], R.GATV2, stats=True),
            T.rel(G["none"], R.GATV2, bias=True, stats=True), T.rel(G["rand"], R.GAT, stats=True, act=1)]
    data = T.draw([("B", T.NB, combine, rels)], H, C, "fold", combine)
    plans = A.Plans(lib)
    try:
        full = _run(lib, T.case("full", (), data, H, C), plans)
        again = _run(lib, T.case("again", (), data, H, C), plans)
        for k in full:
            np.testing.assert_array_equal(_bits(again[k]), _bits(full[k]), err_msg=f"'{k}' differs between two calls")
        name, n_dst, _, drawn = data[0]
        quiet = _run(lib, T.case("quiet", (), [(name, n_dst, combine, [dict(x, stats=False) for x in drawn])], H, C), plans)
        assert set(quiet) == {"out_B"}
        np.testing.assert_array_equal(_bits(quiet["out_B"]), _bits(full["out_B"]), err_msg="out differs with and without stats")
        terms = []
        for j, x in enumerate(drawn):
            one = _run(lib, T.case(f"single{j}", (), [(name, n_dst, combine, [x])], H, C), plans)
            terms.append(one["out_B"])
            if x["g"] is not None:
                np.testing.assert_array_equal(_bits(one["stats_B0"]), _bits(full[f"stats_B{j}"]), err_msg=f"stats of relation {j}")
        want = _fold32(terms, combine)
        same = (_bits(want) == _bits(full["out_B"])) | (np.isnan(want) & np.isnan(full["out_B"]))
        assert same.all(), f"{int((~same).sum())} element(s) differ from the fold of the single-relation calls"
    finally:
        plans.close()


RANGE_HC = (4, 8)


def _range_data(mode):
    """two relations into B whose `a` is scaled so that the largest |logit| of each is 80: both logits are positively homogeneous in `a`
    (GAT: lrelu(a . [Q_i; K_j]), GATv2: a . lrelu(Q_i + K_j)), so the factor is 80 over the largest |logit| of the drawn `a`, taken from
    the float64 restatement.  Returns (drawn call, [float64 logits per relation])"""
    G = T.graphs()
    H, C = RANGE_HC
    data = T.draw([("B", T.NB, T.SUM, [T.rel(G["main"], mode, stats=True), T.rel(G["rand"], mode, bias=True, stats=True)])], H, C, "range", mode)
    logits = lambda x: R._logits(x["g"].s - 1, x["g"].t - 1, x["Q"].astype(np.float64), x["K"].astype(np.float64), x["a"], mode, T.SLOPE, H, C)      # noqa: E731
    ls = []
    for x in data[0][3]:
        x["a"] = (x["a"] * np.float32(80.0 / np.abs(logits(x)).max())).astype(np.float32)
        ls.append(logits(x))
    return data, ls


@pytest.mark.parametrize("mode", [R.GAT, R.GATV2])
def test_the_range_case_reaches_logits_of_80(mode):
    """the set-up of the GPU range test, checked without a GPU: the largest |logit| of either relation is 80 to float32 rounding of `a`,
    the logits of one destination row spread over tens of units, and the float64 reference stays finite"""
    data, ls = _range_data(mode)
    for l in ls:
        assert 79.9 <= np.abs(l).max() <= 80.1, np.abs(l).max()
        assert l.max() - l.min() > 40.0
    want = T.reference(data, *RANGE_HC)
    assert all(not np.isnan(v).any() for v in want.values()) and np.isfinite(want["out_B"]).all()


@gpu
@pytest.mark.parametrize("mode", [R.GAT, R.GATV2])
def test_logits_of_about_80_stay_finite_and_within_the_bar(lib, mode):
    """`a` scaled so that the logits reach 80 in magnitude: the online softmax neither overflows nor loses the bar"""
    H, C = RANGE_HC
    data, ls = _range_data(mode)
    assert all(79.9 <= np.abs(l).max() <= 80.1 for l in ls)
    plans = A.Plans(lib)
    try:
        got = _run(lib, T.case("range", (), data, H, C), plans)
    finally:
        plans.close()
    assert np.isfinite(got["out_B"]).all()
    assert all(np.isfinite(v[..., 1]).all() and not np.isnan(v).any() for k, v in got.items() if k.startswith("stats"))
