"""ppr_diffusion on the device (gnnmp/transform.py, csrc/ppr.hip) against the numpy restatements of the reference (tests/ppr_ref.py, pinned
and checked for conditioning in tests/test_ppr_ref.py).

THE BAR (tests/ppr_ref.py): element-wise |got - ref64| <= K * max(max|lapack32 - ref64|, 2^-24 max|ref64|) with K = 15, a figure taken
from the float32 restatement of the elimination and from LAPACK on the CPU, never from a device.

  * member graphs of 1, 2, 5, 12, 33, 64, 65 and 127 nodes alone, a batch of all of them with two empty members, with and without
    weights (multi-edges, self loops, isolated nodes), index width 4 and 8, index base 0 and 1;
  * the scratch path gives the bits of the LDS path (a graph of 150 nodes too, in LDS only with more than the static 64 KB), and a
    member alone the bits of the same member inside the batch;
  * one graph of 300 nodes (scratch path at the default budget, 300 pivot steps);
  * the pivoting case and alpha = 1, exactly, on both paths; a 70-node elimination that exchanges rows at 63 of its steps;
  * a singular block is a ValueError that names the member graph — a refusal, not a fault: the next call is correct;
  * an edge between two member graphs and a graph_ptr that does not ascend are refused with out untouched;
  * the result graph shares the parent's plans and carries its features and indicator."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_cases as A  # noqa: E402
import ppr_cases  # noqa: E402, F401  (registers the export's cases in A.PREP_TABLE)
import ppr_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32
SCRATCH_FROM_12 = 4 * (11 * 11 + 2 * 11)      # lds_budget_bytes that holds 11 nodes: members of 12 and more take the scratch path
ALL_SCRATCH = 1                               # holds no graph at all
IDX = ((np.int64, 1), (np.int32, 1), (np.int64, 0), (np.int32, 0))


def graph_of(g, idx=np.int64, base=1, **kw):
    import gnnmp
    import torch
    s, t, n, w = g
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return gnnmp.GNNGraph(dev((s + base).astype(idx)), dev((t + base).astype(idx)), None if w is None else dev(w), num_nodes=n,
                          index_base=base, **kw)


def host(x):
    return x.detach().cpu().numpy()


def assert_bar(got, name):
    g, alpha, r64, lap = R.references()[name]
    assert got.shape == r64.shape and got.dtype == f32, name
    ra = R.ratio(got, lap, r64)
    print(f"{name}: {ra:.3f} times the reference's own float32 error (bar {R.K})")
    assert np.all(np.isfinite(got)) and ra <= R.K, (name, ra)
    assert R.within_bar(got, lap, r64)


def slab_of(g, off=None, ib=8, shifts=None):
    arrs = []
    if g[3] is not None:
        arrs.append(A.Arr("w", "in", g[3]))
    if off is not None:
        arrs.append(A.Arr("graph_ptr", "in", np.asarray(off).astype(np.int64 if ib == 8 else np.int32)))
    arrs.append(A.Arr("out", "out", shape=(len(g[0]),)))
    return A.Slab(arrs, shifts=shifts)


def abi_call(gg, slab, alpha, G=1, ib=8, budget=0):
    """the C ABI on the arrays of a slab (w, graph_ptr, out) and the transposed plan of the device graph gg"""
    from gnnmp import _lib
    ptr = lambda name: slab.ptr(name) if name in slab.arrs else None
    job = _lib.PprJob(ptr("w"), ptr("graph_ptr"), ib, G, alpha, budget, slab.ptr("out"))
    return _lib.load().gnnmp_ppr_diffusion_f32(gg.plan_transposed().handle, ctypes.byref(job), _lib.stream_ptr())


def out_of(slab):
    return slab.get(slab.t.cpu().numpy(), "out").copy()


def run_abi(gg, g, alpha, off=None, ib=8, budget=0):
    slab = slab_of(g, off, ib)
    rc = abi_call(gg, slab, alpha, G=1 if off is None else len(off) - 1, ib=ib, budget=budget)
    assert rc == 0, rc
    assert slab.check({"out": A.E(pred=lambda got: None)}) == []          # every element written, nothing else
    return out_of(slab)


def bits(x):
    return np.ascontiguousarray(x, f32).view(np.uint32)


# ---- the device against ref64 -----------------------------------------------------------------------------------------------------------
MEMBER_NAMES = [f"n{n}_{tag}" for tag in "uw" for n in R.SIZES]


@pytest.mark.parametrize("k,name", list(enumerate(MEMBER_NAMES)), ids=MEMBER_NAMES)
def test_a_member_graph_alone(k, name):
    import gnnmp
    g, alpha, _, _ = R.references()[name]
    idx, base = IDX[k % 4]
    gg = graph_of(g, idx, base)
    g2 = gnnmp.ppr_diffusion(gg, alpha)
    assert g2.w.is_cuda and str(g2.w.dtype) == "torch.float32" and tuple(g2.w.shape) == (len(g[0]),)
    got = host(g2.w)
    assert_bar(got, name)
    if g[2] >= 5:                                                          # edge 1 repeats edge 0: every copy receives the same value
        assert got[0] == got[1]
    assert np.array_equal(bits(got), bits(host(gnnmp.ppr_diffusion(gg, alpha).w)))      # deterministic


@pytest.mark.parametrize("weights", [False, True], ids=["unit", "weighted"])
def test_the_batch_with_two_empty_members(weights):
    import gnnmp
    name = "batch_w" if weights else "batch_u"
    g, off, eoff = R.batch(weights)
    ms = R.members(weights)
    gg = graph_of(g)
    outs = {}
    for ib in (8, 4):
        outs[ib] = run_abi(gg, g, R.ALPHA, off, ib)
        assert_bar(outs[ib], name)
    assert np.array_equal(bits(outs[8]), bits(outs[4]))
    # a member alone gives the bits of the same member inside the batch
    for i, m in enumerate(ms):
        alone = host(gnnmp.ppr_diffusion(graph_of(m, *IDX[i % 4]), R.ALPHA).w)
        assert np.array_equal(bits(alone), bits(outs[8][eoff[i]:eoff[i + 1]])), (name, i, m[2])
    # and through the mirror: MLUtils.batch of the members, and an indicator that skips the ids of the two empty members
    gb = gnnmp.batch([graph_of(m) for m in ms])
    assert gb.num_graphs == len(ms)
    assert np.array_equal(bits(host(gnnmp.ppr_diffusion(gb, R.ALPHA).w)), bits(outs[8]))
    import torch
    ids = np.repeat(np.arange(1, len(off)), np.diff(off))
    gi = graph_of(g, graph_indicator=torch.from_numpy(ids).cuda(), num_graphs=len(off) - 1)
    assert np.array_equal(bits(host(gnnmp.ppr_diffusion(gi, R.ALPHA).w)), bits(outs[8]))


# ---- both paths, the same bits ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["batch_u", "batch_w", "n65_u", "n65_w", "n127_u", "n127_w", "n150_w"])
def test_the_scratch_path_gives_the_bits_of_the_lds_path(name):
    import gnnmp
    g, alpha, _, _ = R.references()[name]
    off = R.batch(name.endswith("w"))[1] if name.startswith("batch") else None
    assert SCRATCH_FROM_12 < 4 * (12 * 12 + 2 * 12)
    gg = graph_of(g)
    # (n150_w: 150 nodes are above the default budget — the default is its scratch path, and 160 KB, which the launch has to opt
    # into, its LDS path)
    lds = run_abi(gg, g, alpha, off, budget=0)
    assert_bar(lds, name)
    for budget in (SCRATCH_FROM_12, ALL_SCRATCH, 160 * 1024):
        assert np.array_equal(bits(run_abi(gg, g, alpha, off, budget=budget)), bits(lds)), (name, budget)
    # the mirror passes the field through
    assert np.array_equal(bits(host(gnnmp.ppr_diffusion(gg, alpha, lds_budget_bytes=SCRATCH_FROM_12).w)), bits(lds))
    if off is not None:
        # without graph_ptr the batch is ONE graph of 309 nodes (block diagonal, scratch path): the same bits again
        assert np.array_equal(bits(run_abi(gg, g, alpha)), bits(lds))


def test_one_graph_of_300_nodes_takes_the_scratch_path_at_the_default_budget():
    import gnnmp
    g, alpha, _, _ = R.references()["large300_w"]
    assert 4 * (300 * 300 + 600) > 160 * 1024
    gg = graph_of(g)
    got = run_abi(gg, g, alpha, budget=0)                                     # the record's default: 64 KB
    assert_bar(got, "large300_w")
    assert np.array_equal(bits(host(gnnmp.ppr_diffusion(gg, alpha).w)), bits(got))      # the mirror (it asks for 160 KB): scratch all the same


# ---- exact cases --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("budget", [0, ALL_SCRATCH], ids=["lds", "scratch"])
def test_the_pivoting_case_and_alpha_one(budget):
    import gnnmp
    g, alpha = R.PIVOT
    got = host(gnnmp.ppr_diffusion(graph_of(g), alpha, lds_budget_bytes=budget).w)
    assert np.array_equal(got, R.PIVOT_ANSWER)
    assert_bar(got, "pivot")
    g, alpha = R.known_cases()["alpha1"]
    got = host(gnnmp.ppr_diffusion(graph_of(g), alpha, lds_budget_bytes=budget).w)
    assert np.array_equal(got, (g[0] == g[1]).astype(f32))                 # 1 on self loops, 0 elsewhere
    g, alpha = R.TWO_CYCLE
    got = host(gnnmp.ppr_diffusion(graph_of(g), alpha, lds_budget_bytes=budget).w)
    assert_bar(got, "two_cycle")
    # an integer alpha is a real number too; a graph without edges comes back with an empty weight vector
    g1 = R.known_cases()["alpha1"][0]
    assert np.array_equal(host(gnnmp.ppr_diffusion(graph_of(g1), 1, lds_budget_bytes=budget).w), (g1[0] == g1[1]).astype(f32))
    empty = gnnmp.ppr_diffusion(graph_of(R._g([], [], 3)), 0.85)
    assert tuple(empty.w.shape) == (0,) and empty.num_nodes == 3


def test_an_elimination_that_exchanges_rows_at_almost_every_step():
    """exchange70 (tests/ppr_ref.py): 63 exchanges in 70 steps, pivots found beyond the first 64 rows — the cross-lane and cross-wave pivot
    reduction, the old a_kk taken for the row that came from k, and a column map of many exchanges, on both paths, alone and in a batch"""
    import gnnmp
    import torch
    g, alpha, _, _ = R.references()["exchange70"]
    gg = graph_of(g)
    lds = run_abi(gg, g, alpha, budget=0)
    assert_bar(lds, "exchange70")
    for budget in (SCRATCH_FROM_12, ALL_SCRATCH):
        assert np.array_equal(bits(run_abi(gg, g, alpha, budget=budget)), bits(lds)), budget
    # between two other members (the pivot rows are then offset inside the batch; 1024 threads a workgroup as alone)
    two = R._g([0, 1], [1, 0], 2, [1.0, 1.0])
    gb, off = R.concat([two, g, R.PIVOT[0]])
    ids = torch.from_numpy(np.repeat(np.arange(1, 4), np.diff(off))).cuda()
    ggb = graph_of(gb, np.int32, 1, graph_indicator=ids, num_graphs=3)
    for budget in (160 * 1024, SCRATCH_FROM_12):
        got = host(gnnmp.ppr_diffusion(ggb, alpha, lds_budget_bytes=budget).w)
        assert np.array_equal(bits(got[2:2 + len(g[0])]), bits(lds)), budget
        assert np.array_equal(got[2 + len(g[0]):], R.PIVOT_ANSWER), budget


# ---- singular: a refusal, not a fault ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("budget", [0, ALL_SCRATCH], ids=["lds", "scratch"])
def test_a_singular_block_is_a_value_error_that_names_the_member(budget):
    import gnnmp
    import torch
    from gnnmp import _lib
    g, alpha = R.SINGULAR
    with pytest.raises(ValueError, match="member graph 0 is singular"):
        gnnmp.ppr_diffusion(graph_of(g), alpha, lds_budget_bytes=budget)
    # inside a batch: the pivoting case (fine), the singular node, the two-cycle (fine)
    gb, off = R.concat([R.PIVOT[0], R.SINGULAR[0], R._g([0, 1], [1, 0], 2, [1.0, 1.0])])
    ids = torch.from_numpy(np.repeat(np.arange(1, 4), np.diff(off))).cuda()
    ggb = graph_of(gb, graph_indicator=ids, num_graphs=3)
    with pytest.raises(ValueError, match="member graph 1 is singular"):
        gnnmp.ppr_diffusion(ggb, alpha, lds_budget_bytes=budget)
    slab = slab_of(gb, off)
    assert abi_call(ggb, slab, alpha, G=3, budget=budget) == _lib.EINVAL
    assert b"member graph 1" in _lib.load().gnnmp_last_error()
    # out is unspecified then (elements may or may not have been written); nothing outside it was touched
    assert [p for p in slab.check({"out": A.E(pred=lambda got: None)}) if "never written" not in p] == []
    # the call afterwards, on a good graph, is correct
    g, alpha = R.PIVOT
    assert np.array_equal(host(gnnmp.ppr_diffusion(graph_of(g), alpha, lds_budget_bytes=budget).w), R.PIVOT_ANSWER)
    got = host(gnnmp.ppr_diffusion(graph_of(R.references()["n33_w"][0]), R.ALPHA, lds_budget_bytes=budget).w)
    assert_bar(got, "n33_w")


# ---- the check launch -------------------------------------------------------------------------------------------------------------------
def test_an_edge_between_two_graphs_and_an_unsorted_indicator_are_refused():
    import gnnmp
    import torch
    from gnnmp import _lib
    (s, t, n, w), off, _ = R.batch(True)
    t = t.copy()
    e = int(np.flatnonzero(s >= off[2])[0])                                   # an edge of the 5-node member ...
    t[e] = off[4]                                                             # ... now ends in the first node of the 12-node member
    g = (s, t, n, w)
    ids = torch.from_numpy(np.repeat(np.arange(1, len(off)), np.diff(off))).cuda()
    gg = graph_of(g, graph_indicator=ids, num_graphs=len(off) - 1)
    with pytest.raises(ValueError, match="leaves its graph"):
        gnnmp.ppr_diffusion(gg, R.ALPHA)
    for budget in (0, ALL_SCRATCH):
        slab = slab_of(g, off)                                                # out starts as a fixed pattern: it must come back untouched
        assert abi_call(gg, slab, R.ALPHA, G=len(off) - 1, budget=budget) == _lib.EINVAL
        assert b"leaves its graph" in _lib.load().gnnmp_last_error()
        assert slab.check({}, untouched=True) == []
    # the same edge list is a fine single graph
    one = host(gnnmp.ppr_diffusion(graph_of(g), R.ALPHA).w)
    assert R.within_bar(one, R.lapack32(*g, R.ALPHA), R.ref64(*g, R.ALPHA))
    # an indicator that is not sorted: 0 -> 2 and 1 -> 3 with the nodes labelled 1, 2, 1, 2 — whichever boundary the offsets get, one of
    # the two edges crosses it
    bad = graph_of(R._g([0, 1], [2, 3], 4), graph_indicator=torch.tensor([1, 2, 1, 2]).cuda(), num_graphs=2)
    with pytest.raises(ValueError, match="leaves its graph|graph_ptr"):
        gnnmp.ppr_diffusion(bad, R.ALPHA)
    # a graph_ptr that does not ascend from 0 to N, at both widths
    g0, off0, _ = R.batch(False)
    gg0 = graph_of(g0)
    short, late, down = off0.copy(), off0.copy(), off0.copy()
    short[-1] -= 1
    late[0] = 1
    down[5], down[6] = off0[6], off0[5]
    for ib in (8, 4):
        for what, ptr in (("short", short), ("late", late), ("down", down)):
            slab = slab_of(g0, ptr, ib)
            assert abi_call(gg0, slab, R.ALPHA, G=len(off0) - 1, ib=ib) == _lib.EINVAL, what
            assert b"graph_ptr" in _lib.load().gnnmp_last_error(), what
            assert slab.check({}, untouched=True) == [], what


# ---- the result graph -------------------------------------------------------------------------------------------------------------------
def test_the_result_graph_shares_the_plans_and_carries_the_features():
    import gnnmp
    import torch
    ms = R.members(True)[2:6]                                                 # 5, 12, 33 and 64 nodes
    (s, t, n, w), off = R.concat(ms)
    ids = torch.from_numpy(np.repeat(np.arange(1, len(ms) + 1), np.diff(off))).cuda()
    x = torch.from_numpy(np.random.default_rng(3).standard_normal((n, 7)).astype(f32)).cuda()
    g = graph_of((s, t, n, w), graph_indicator=ids, num_graphs=len(ms), x=x)
    plan = g.plan(False)
    g2 = gnnmp.ppr_diffusion(g)                                               # alpha = 0.85, the reference's default
    assert g2._plans is g._plans and g2.plan(False) is plan and g2.plan_transposed() is g.plan_transposed()
    assert g2._cache["node_ptr"] is g._cache["node_ptr"]                      # the node offsets too: the same nodes and indicator
    with pytest.raises(TypeError):
        gnnmp.ppr_diffusion(g, 0.85, 0)                                       # the budget is keyword only
    assert g2.s is g.s and g2.t is g.t and g2.x is g.x and g2.graph_indicator is g.graph_indicator
    assert (g2.num_nodes, g2.num_edges, g2.num_graphs, g2.index_base) == (g.num_nodes, g.num_edges, g.num_graphs, g.index_base)
    assert g.w is not None and g2.w is not g.w and np.array_equal(host(g.w), w)           # the parent keeps its weights
    assert R.within_bar(host(g2.w), R.lapack32(s, t, n, w, 0.85), R.ref64(s, t, n, w, 0.85))
    y2 = gnnmp.propagate(gnnmp.w_mul_xj, g2, "+", xj=x)
    y1 = gnnmp.propagate(gnnmp.e_mul_xj, g, "+", xj=x, e=g2.w)               # the new weights passed explicitly, on the parent
    assert np.array_equal(bits(host(y2)), bits(host(y1)))
    ref = np.zeros((n, 7))
    np.add.at(ref, t, host(g2.w).astype(np.float64)[:, None] * host(x).astype(np.float64)[s])
    assert np.abs(host(y2) - ref).max() <= 1e-5 * np.abs(ref).max()
    # a graph without weights yields a weighted graph
    gu = graph_of((s, t, n, None))
    assert gu.w is None and gnnmp.ppr_diffusion(gu).w is not None
