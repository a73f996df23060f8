"""The row walk under every geometry knob (csrc/rowwalk.h: decode_vrow, row_grid; csrc/csr_reduce.h: reduce_range).

csrc/knobs.h promises that every knob value selects correct code.  The knobs that shape the walk — FORCE_LOG2G (lanes per row, hence
feature tiles), UNROLL (batch depth), XCD_REMAP (block -> virtual-row map), BLOCK_WAVES (rows per block), ROW_ORDER (rows walked through
plan->row_order) — select kernel instances and host branches that the default geometry never reaches.  Two sweeps, both through the raw
C ABI on poisoned slabs (tests/abi_cases.py), never through the Python wrappers: their outputs come from torch's caching allocator, and a
row a kernel skipped under a knob would inherit the right value from the previous call's freed buffer.

  Part A  every case of every export of the ABI case table with the lane group forced to 1, 8 and 64 lanes;
  Part B  a graph built for the walk's edges (abi_cases.GeomCtx) through the kernels that remap, reorder and batch, under each knob
          alone and in three combinations: against the case's reference, and bit for bit against the default geometry where the knob
          only changes which lane group takes which row.

Every bound is the case table's own (exact, 1e-5 of the reference's scale, exact_rows)."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_cases as A  # noqa: E402

gpu = pytest.mark.gpu

FORCE_VEC, FORCE_LOG2G, UNROLL, XCD_REMAP, BLOCK_WAVES, FUSED_WAVES, ROW_ORDER, SOFTMAX_ROWS, VARIANT = 0, 1, 2, 3, 5, 14, 15, 16, 19
KNOB_NAMES = {FORCE_LOG2G: "FORCE_LOG2G", UNROLL: "UNROLL", XCD_REMAP: "XCD_REMAP", BLOCK_WAVES: "BLOCK_WAVES", FUSED_WAVES: "FUSED_WAVES",
              ROW_ORDER: "ROW_ORDER", SOFTMAX_ROWS: "SOFTMAX_ROWS", VARIANT: "VARIANT"}
TWO_KERNEL_FOLD = 128           # csrc/knobs.h: VARIANT_TWO_KERNEL_FOLD


@pytest.fixture(scope="module")
def lib():
    import torch
    assert torch.cuda.is_available()
    from gnnmp import _lib
    return _lib.load()


def _dry_thr():
    _, defines = A.parse_header()
    return int(defines["GNNMP_MIN_LONG_ROW"])


def _fail(case, what, problems):
    return f"{case.export}[{case.sid}] {what}:\n  " + "\n  ".join(problems)


def _overlaid(case, knobs):
    """the same case with `knobs` laid over its own (abi_cases.call applies them and puts the previous values back)"""
    c = A.Case(case.export, case.sid, case.args, case.ref, guard=case.guard, status=case.status, align_status=case.align_status,
               knobs={**case.knobs, **knobs}, no_warmup=case.no_warmup)
    c.tags = getattr(case, "tags", set())
    return c


# ------------------------------------------------------------------------------------------------------------------------------------
# Part A: the whole case table under a forced lane group
# ------------------------------------------------------------------------------------------------------------------------------------
# An export whose default status is OK may answer GNNMP_EUNSUPPORTED under a forced lane group only if it is listed here, and then
# nothing may have been written.  Every entry has its reason in the text of knob 1 in csrc/knobs.h and a host-side refusal:
#   gnnmp_fused_conv_f32   fused_conv_kernel / fused_cat_kernel have no feature tiles (a lane stores its features to the LDS tile once)
MAY_REFUSE_FORCED_GROUP = {"gnnmp_fused_conv_f32"}

FORCED = (0, 3, 6)              # one lane a row: feature tiles everywhere; 8 lanes; a whole wave a row: idle lanes everywhere


@pytest.fixture(scope="module")
def table_ctx(lib):
    return A.Ctx(A.plan_threshold(lib, A.Ctx(_dry_thr()).hub.E))


def _leaf_and_dense_exports():
    """the exports defined in csrc/leaf.hip and csrc/dense*.hip: elementwise, gather, segment-pool and GEMM entry points"""
    import glob
    import re
    csrc = os.path.join(A.ROOT, "graphneuralnetworks.jl_amd", "csrc")
    names = set()
    for path in [os.path.join(csrc, "leaf.hip")] + sorted(glob.glob(os.path.join(csrc, "dense*.hip"))):
        names |= set(re.findall(r"^(?:extern \"C\" )?int (gnnmp_\w+)\(", open(path).read(), flags=re.M))
    return names & set(A.TABLE)


# Thinned, because three unshifted passes of the table took longer than tests/test_abi_memory_contract.py (9.5 s against 6.9 s on one
# MI355X): the leaf and dense exports run at the two extremes only.  Every other export — every one whose host path asks pick_log2g or
# row_walk_geom for a row walk, plans inside records (hetero) included — runs at all three values.  No export is dropped.  Part A
# stays the longer of the two (10.0 s against 7.0 s): gnnmp_segment_attn_pool(_grad)_f32 with one lane a row alone take 4 s.
LEAF_AND_DENSE = _leaf_and_dense_exports()
FORCED_CASES = [(e, v) for e in sorted(A.TABLE) for v in FORCED if v != 3 or e not in LEAF_AND_DENSE]


@gpu
@pytest.mark.parametrize("export,log2g", FORCED_CASES)
def test_case_table_under_a_forced_lane_group(lib, table_ctx, export, log2g):
    plans = A.Plans(lib)
    failures = []
    try:
        for case in A.TABLE[export](table_ctx):
            forced = _overlaid(case, {FORCE_LOG2G: log2g})
            rc, slab, host = A.run_case(lib, forced, plans)
            if rc == A.EUNSUPPORTED and case.status == A.OK and export in MAY_REFUSE_FORCED_GROUP:
                problems = slab.check({}, untouched=True)              # a documented refusal: nothing may have been written
            else:
                problems = A.verify(forced, rc, slab, host)
                if rc != case.status:
                    problems = [f"status {rc} ({lib.gnnmp_last_error().decode()}), the default geometry gives {case.status}"]
            if problems:
                failures.append(_fail(case, f"FORCE_LOG2G = {log2g}", problems))
    finally:
        plans.close()
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------------------------------------------------------------------------------
# Part B: a graph built for the walk's edges through the kernels that remap, reorder and batch
# ------------------------------------------------------------------------------------------------------------------------------------
KNOB_SETS = {
    "default": {},                  # the geometry the library picks: against the reference, and the same bytes twice
    "unroll2": {UNROLL: 2}, "unroll4": {UNROLL: 4},
    "waves1": {BLOCK_WAVES: 1}, "waves2": {BLOCK_WAVES: 2}, "waves3": {BLOCK_WAVES: 3},
    "remap0": {XCD_REMAP: 0}, "remap2": {XCD_REMAP: 2},
    "order2": {ROW_ORDER: 2},
    "group1": {FORCE_LOG2G: 0}, "group64": {FORCE_LOG2G: 6},
    "order2+remap2+waves3": {ROW_ORDER: 2, XCD_REMAP: 2, BLOCK_WAVES: 3},
    "unroll2+group64": {UNROLL: 2, FORCE_LOG2G: 6},
    "fold2k+order2": {VARIANT: TWO_KERNEL_FOLD, ROW_ORDER: 2},
}

PROPAGATE = ("gnnmp_propagate_f32", "gnnmp_propagate_slots_f32", "gnnmp_propagate_slots_act_f32", "gnnmp_propagate_add_mask_f32",
             "gnnmp_propagate_emul_f32", "gnnmp_propagate_gated_f32", "gnnmp_propagate_cg_f32", "gnnmp_propagate_nn_f32", "gnnmp_scatter_f32")
ATTENTION = ("gnnmp_gat_conv_f32", "gnnmp_gat_conv_stats_f32", "gnnmp_gat_conv_train_f32", "gnnmp_gat_conv_edge_f32", "gnnmp_gat_conv_drop_f32",
             "gnnmp_attn_conv_f32", "gnnmp_gat_aggregate_f32", "gnnmp_gat_conv_grad_f32", "gnnmp_gat_conv_grad2_f32", "gnnmp_gat_conv_grad_drop_f32")
# (the table's export, the knobs laid under every knob set): the edge softmax in both settings of SOFTMAX_ROWS
TARGETS = {e: (e, {}) for e in PROPAGATE + ATTENTION + ("gnnmp_fused_conv_f32",)}
TARGETS["gnnmp_edge_softmax_f32"] = ("gnnmp_edge_softmax_f32", {SOFTMAX_ROWS: 0})
TARGETS["gnnmp_edge_softmax_f32/three-step"] = ("gnnmp_edge_softmax_f32", {SOFTMAX_ROWS: -1})

# Knobs that only change WHICH lane group takes which row (the block -> row map, the rows of a block, the order of the rows): the edge
# order inside a row, the chunk boundaries (plan build) and the fold order of the chunks stay, so every output byte must equal the
# default geometry's.
PLACEMENT = {BLOCK_WAVES, XCD_REMAP, ROW_ORDER}
# The propagate family adds its edges one at a time in slot order whatever the batch depth, and the in-kernel fold is built to equal
# the combine kernel bit for bit (tests/test_fold_in_kernel.py): UNROLL and the two-kernel fold must not change a byte either.
PROPAGATE_ALSO = {UNROLL, VARIANT}
# (target, knob set) pairs moved from "bit-identical to the default geometry" to "reference only", each with the reason in the code
REFERENCE_ONLY = {}


def must_be_identical(target, kset):
    if (target, kset) in REFERENCE_ONLY:
        return False
    knobs = set(KNOB_SETS[kset])
    return knobs <= PLACEMENT or (target in PROPAGATE and knobs <= PLACEMENT | PROPAGATE_ALSO)


def claimed_walks(ctx):
    """(what, graph, plan-added self loops, row width, head width, waves a block by default, split rows are chunk virtual rows) of every
    row walk of Part B whose host path asks use_xcd_remap (lane groups from abi_cases.lanes_of: pick_vec at the slab's 256-byte aligned
    pointers, where narrow_vec — emul, gated, cg, add_mask — narrows nothing, so one geometry a width holds for the whole family): run_reduce (csrc/propagate.hip) for the propagate family, launch_gat_fused
    (csrc/gat_fused.hip) for the one-pass attention forward, launch_gat (csrc/attention.hip) for gnnmp_gat_aggregate_f32, which
    walks split rows whole in a kernel of its own (n_chunks = 0: nothing in front of the remapped blocks)"""
    for g, D in ctx.widths():
        yield "run_reduce", g, False, D, None, 4, True
    for loops in (False, True):
        for g, H, C, _ in ctx.att_shapes(loops):
            yield "gat_fused", g, loops, H * C, C, 1, True
    for g, H, C, _ in ctx.att_shapes(False):
        yield "gat_aggregate", g, False, H * C, C, 1, False


def geometry_problems(ctx):
    """the premises of Part B, from row lengths alone: [] when every claimed (walk, knob set) has at least 64 row blocks (below that
    use_xcd_remap says no even at knob = 2), chunk blocks in front (nbc > 0), a number of ordinary-row blocks that is no multiple of 8
    (the grid is padded) and a partly empty last block.  Knob sets that force the lane group are not claimed"""
    problems = []
    for what, g, loops, width, C, waves0, chunked in claimed_walks(ctx):
        _, log2g = A.lanes_of(width, C)
        lengths = g.indeg() + (1 if loops else 0)
        n_chunks = A.n_chunks_of(lengths, ctx.thr) if chunked else 0
        for kset, knobs in KNOB_SETS.items():
            if FORCE_LOG2G in knobs:
                continue
            waves = knobs.get(BLOCK_WAVES, waves0)
            blocks, nbc, last, rpb = A.walk_blocks(g.n_dst, n_chunks, log2g, waves)
            bad = []
            if -(-g.n_dst // rpb) < 64:                                # blocks >= ceil(n_dst / rows per block): no plan internals
                bad.append(f"{-(-g.n_dst // rpb)} row blocks < 64")
            if (blocks - nbc) % 8 == 0:
                bad.append(f"{blocks - nbc} ordinary-row blocks: a multiple of 8, no padding")
            if chunked and nbc == 0:
                bad.append("no chunk blocks")
            if chunked and rpb > 1 and last == rpb:
                bad.append("the last block is full")
            if bad:
                problems.append(f"{what} on {g.name} (loops {loops}), width {width}, {kset}: " + "; ".join(bad))
    return problems


def test_the_geometry_graphs_have_the_rows_and_block_counts_the_sweep_is_about():
    """CPU: with the header's GNNMP_MIN_LONG_ROW as the threshold (as the table's dry run)"""
    from gnnmp.knobs import Knob
    thr = _dry_thr()
    ctx = A.GeomCtx(thr)
    for g in (ctx.wide, ctx.narrow):
        deg = g.indeg()
        assert deg[0] == 0 and deg[-1] == 0 and deg[g.n // 2] == 0
        assert set(A.geom_lengths(thr)) <= set(deg.tolist()), sorted(set(A.geom_lengths(thr)) - set(deg.tolist()))
        assert {thr - 1, thr, thr + 1, 5 * thr + 3} <= set(deg.tolist())
        assert -(-int(deg.max()) // min(thr, A.CHUNK_SLOTS)) > A.GEOM_HUB_CHUNKS                 # the large hub: more than 20 chunks
        assert all(int(deg[row]) == length for length, row in g.at.items())
        for length in (8, 16):                                                                   # multi-edges
            assert len(set(g.s[g.t == g.at[length] + 1].tolist())) == 1
        out = np.bincount(g.s - 1, minlength=g.n)
        assert out.max() > thr + 1 and (out == 0).any()                   # the transposed plan: a split row, and empty rows
        # plan->row_order begins with the split rows, which every row kernel skips: three of them without plan-added self loops, so that
        # the positions from 3 on are ordinary rows and a walk that loses one of the first few positions loses a row
        assert g.want_split == int((deg > thr).sum()) == 3 and np.sort(deg)[-4] == thr
    assert geometry_problems(ctx) == []
    for knobs in KNOB_SETS.values():
        for k in knobs:
            assert Knob[KNOB_NAMES[k]] == k
    assert Knob["SOFTMAX_ROWS"] == SOFTMAX_ROWS and Knob["FUSED_WAVES"] == FUSED_WAVES
    # every target has cases on both graphs' kinds of row, and the fused kernel keeps its own knob
    for target, (export, under) in TARGETS.items():
        cases = A.TABLE[export](ctx)
        assert len(cases) >= 3 and len({c.sid for c in cases}) == len(cases), target
    assert all(c.knobs == {FUSED_WAVES: 16} for c in A.TABLE["gnnmp_fused_conv_f32"](ctx))
    # the table's own data is what it was: the builders' hooks change nothing for a Ctx
    t = A.Ctx(thr)
    assert [c.sid for c in A.TABLE["gnnmp_propagate_nn_f32"](t)][:2] == ["hub_3x5_a0", "hub_4x4_a1"]
    assert len(A.TABLE["gnnmp_fused_conv_f32"](t)) == 8 and len(A.TABLE["gnnmp_edge_softmax_f32"](t)) == 20


class Geom:
    """the cases of Part B, built once: every reference is computed once and shared by the knob sets, like the bytes of the
    default-geometry run of every case"""

    def __init__(self, lib):
        self.ctx = A.GeomCtx(A.plan_threshold(lib, A.GeomCtx(_dry_thr()).narrow.E))
        self.cases, self.default = {}, {}

    def of(self, export):
        if export not in self.cases:
            self.cases[export] = cs = A.TABLE[export](self.ctx)
            for c in cs:
                c.ref = self._once(c.ref)
        return self.cases[export]

    @staticmethod
    def _once(ref):
        memo = []
        def cached(host):
            if not memo:
                memo.append(ref(host))
            return memo[0]
        return cached

    def default_bytes(self, lib, target, case, under):
        key = (target, case.sid)
        if key not in self.default:
            plans = A.Plans(lib)
            try:
                rc, slab, host = A.run_case(lib, _overlaid(case, under), plans)
                assert rc == case.status, (target, case.sid, rc)
                self.default[key] = slab.outputs()
            finally:
                plans.close()
        return self.default[key]


@pytest.fixture(scope="module")
def geom(lib):
    return Geom(lib)


@gpu
def test_the_geometry_is_reached_on_the_device(lib, geom):
    """the same premises with the threshold the library gives these plans, and the plans themselves: the forward plans split the rows
    the graphs were built to have split (abi_cases.Plans asserts it), the transposed plans split one too"""
    ctx = geom.ctx
    assert geometry_problems(ctx) == []
    plans = A.Plans(lib)
    try:
        for g in (ctx.wide, ctx.narrow):
            plans.get(A.Pl(g))
            for loops in (False, True):
                info = (ctypes.c_int64 * 8)()
                assert lib.gnnmp_plan_info(plans.get(A.Pl(g, T=True, loops=loops)), info) == A.OK
                assert info[7] == ctx.thr and info[5] >= 1, (g.name, loops, list(info))
    finally:
        plans.close()


@gpu
@pytest.mark.parametrize("kset", list(KNOB_SETS))
@pytest.mark.parametrize("target", list(TARGETS))
def test_geometry_graph_under_a_knob_set(lib, geom, target, kset):
    export, under = TARGETS[target]
    identical = must_be_identical(target, kset)
    plans = A.Plans(lib)
    failures = []
    try:
        for case in geom.of(export):
            tuned = _overlaid(case, {**under, **KNOB_SETS[kset]})
            rc, slab, host = A.run_case(lib, tuned, plans)
            if rc == A.EUNSUPPORTED and case.status == A.OK and FORCE_LOG2G in KNOB_SETS[kset] and export in MAY_REFUSE_FORCED_GROUP:
                problems = slab.check({}, untouched=True)
            else:
                problems = A.verify(tuned, rc, slab, host)
                if rc != case.status:
                    problems = [f"status {rc} ({lib.gnnmp_last_error().decode()}), the default geometry gives {case.status}"]
                elif identical:
                    want, got = geom.default_bytes(lib, target, case, under), slab.outputs()
                    for name in want:
                        if not np.array_equal(want[name], got[name]):
                            a = slab.arrs[name]
                            w, g_ = want[name].view(a.dtype), got[name].view(a.dtype)
                            first = int(np.flatnonzero(w.view(np.uint32 if a.dtype.itemsize == 4 else np.uint8) !=
                                                       g_.view(np.uint32 if a.dtype.itemsize == 4 else np.uint8))[0])
                            problems.append(f"output '{name}' is not bit-identical to the default geometry's: first at element {first} "
                                            f"({g_[first]!r} != {w[first]!r})")
            if problems:
                failures.append(_fail(case, kset, problems))
    finally:
        plans.close()
    assert not failures, "\n".join(failures)
