"""random_walk_pe on the device (gnnmp/transform.py, csrc/rwpe.hip) against the numpy restatement of the reference (tests/rwpe_ref.py,
itself pinned to the reference's test item and checked for conditioning in tests/test_rwpe_abi.py):

  * the reference's known answer, exactly, through the mirror and through the C ABI;
  * the semantics the model fixes — a node without out-edges, a self loop, a doubled edge, weights, walk_length = 1, a one-node graph, a
    directed graph — within 1e-5 of the float64 model norm-wise and element by element, with exact zeros where the model has zeros;
  * tiles and batches: member graphs of 1, 2, T - 1, T, T + 1, 2 T + 1 and 65 nodes, bit-identical alone and inside the batch, an empty
    graph in the middle of graph_ptr;
  * the LDS path and the scratch path give the same bits;
  * the check launch refuses an edge between two graphs and a graph_ptr that does not ascend from 0 to N, writing nothing;
  * the memory contract, on the poisoned, guarded, shifted slab of tests/abi_cases.py (the output travels in a const host record, so
    that module's table does not reach the export)."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_cases as A  # noqa: E402
import rwpe_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32


def tile():
    from gnnmp import _lib
    return _lib.RWPE_TILE


def refs():
    return R.references(tile())


def graph_of(g, idx=np.int64, base=1, **kw):
    import gnnmp
    import torch
    s, t, n, w = g
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return gnnmp.GNNGraph(dev((s + base).astype(idx)), dev((t + base).astype(idx)), None if w is None else dev(w), num_nodes=n,
                          index_base=base, **kw)


def host(x):
    return x.detach().cpu().numpy()


def assert_model(got, name):
    g, K, d64, _ = refs()[name]
    assert got.shape == d64.shape and got.dtype == f32, name
    nw, ew = R.deviation(got, d64)
    print(f"{name}: norm-wise {nw:.3g}, element-wise {ew:.3g}")
    assert nw <= R.BAR and ew <= R.BAR, (name, nw, ew)


def abi_call(gg, slab, K, G=1, ib=8, budget=None, w=True, gp=True):
    """the C ABI on the arrays of a slab (w, graph_ptr, out) and the transposed plan of the device graph gg"""
    from gnnmp import _lib
    lib = _lib.load()
    ptr = lambda name, on: slab.ptr(name) if (on and name in slab.arrs) else None
    job = _lib.RwpeJob(ptr("w", w), ptr("graph_ptr", gp), ib, G, K, slab.ptr("out"))
    h = gg.plan_transposed().handle
    if budget is None:
        return lib.gnnmp_random_walk_pe_f32(h, ctypes.byref(job), _lib.stream_ptr())
    return lib.gnnmp_debug_random_walk_pe_f32(h, ctypes.byref(job), budget, _lib.stream_ptr())


def slab_of(g, K, off=None, ib=8, shifts=None):
    arrs = []
    if g[3] is not None:
        arrs.append(A.Arr("w", "in", g[3]))
    if off is not None:
        arrs.append(A.Arr("graph_ptr", "in", np.asarray(off).astype(np.int64 if ib == 8 else np.int32)))
    arrs.append(A.Arr("out", "out", shape=(g[2], K)))
    return A.Slab(arrs, shifts=shifts)


def out_of(slab):
    return slab.get(slab.t.cpu().numpy(), "out").copy()


# ---- known answer ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx,base", [(np.int64, 1), (np.int32, 1), (np.int64, 0)])
def test_known_answer_through_the_mirror(idx, base):
    import gnnmp
    pe = gnnmp.random_walk_pe(graph_of(R.KNOWN, idx, base), 3)
    assert tuple(pe.shape) == (3, 3) and pe.is_cuda and str(pe.dtype) == "torch.float32"
    assert np.array_equal(host(pe), R.KNOWN_ANSWER)
    assert np.array_equal(host(pe).T, np.array([[0, 0, 0], [0.5, 1, 0.5], [0, 0, 0]], f32))       # the reference's (walk_length, N)


def test_known_answer_through_the_c_abi():
    gg = graph_of(R.KNOWN)
    for budget in (None, 0, 1):                               # the export, the internal variant's default, the scratch path
        slab = slab_of(R.KNOWN, 3)
        assert abi_call(gg, slab, 3, budget=budget) == 0
        assert slab.check({"out": A.E(R.KNOWN_ANSWER, "exact")}) == [], budget


# ---- semantics ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.semantic_cases()))
def test_semantics(name):
    import gnnmp
    g, K, d64, _ = refs()[name]
    got = host(gnnmp.random_walk_pe(graph_of(g), K))
    assert_model(got, name)
    if name == "sink":
        assert np.all(got[3] == 0)
    if name == "self_loop":
        assert got[0, 0] == 0.5
    if name == "one_node_loop":
        assert np.all(got == 1)
    if name == "one_node_bare":
        assert np.all(got == 0)
    if name == "directed":
        # the case is not blind: degrees taken from the wrong direction are far outside the bar on it.  (The row-scaled matrix
        # Diagonal(dinv) * A has the same diagonals as the model on every graph — tests/test_rwpe_abi.py pins that identity — so it is
        # not a variant any case could catch.)
        wrong = R.dense64(*g, K, in_degree=True)
        assert R.deviation(wrong, d64)[0] > 1000 * R.BAR
        assert not R.within_bar(got, wrong)


# ---- tiles and batches ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["batch", "batch_weighted"])
def test_batch_matches_the_model_and_every_member_alone(which):
    import gnnmp
    T = tile()
    members = R.batch_members(T) if which == "batch" else R.batch_weighted_members(T)
    gs = [graph_of(m) for m in members]
    gb = gnnmp.batch(gs)
    (s, t, n, w), off = R.concat(members)
    assert gb.num_graphs == len(members) and gb.num_nodes == n and np.array_equal(host(gb.s) - 1, s)
    got = host(gnnmp.random_walk_pe(gb, R.BATCH_WALK))
    assert_model(got, which)
    for i, (m, gm) in enumerate(zip(members, gs)):
        alone = host(gnnmp.random_walk_pe(gm, R.BATCH_WALK))
        assert np.array_equal(alone.view(np.uint32), got[off[i]:off[i + 1]].view(np.uint32)), (which, i, m[2])
        if which == "batch":
            assert_model(alone, f"member{i}")


@pytest.mark.parametrize("ib", [8, 4])
def test_an_empty_graph_in_the_middle_of_graph_ptr(ib):
    T = tile()
    members = R.batch_members(T)
    g, off = R.concat(members)
    off2 = np.concatenate([off[:3], off[2:5], off[4:], off[-1:]])        # empty graphs after the second and fourth member and at the end
    assert len(off2) == len(off) + 3 and np.all(np.diff(off2) >= 0) and np.sum(np.diff(off2) == 0) == 3
    gg = graph_of(g)
    slab = slab_of(g, R.BATCH_WALK, off2, ib)
    assert abi_call(gg, slab, R.BATCH_WALK, G=len(off2) - 1, ib=ib) == 0
    assert slab.check({"out": A.E(pred=lambda got: None)}) == []
    assert_model(out_of(slab), "batch")


# ---- both paths -----------------------------------------------------------------------------------------------------------------------
def test_the_scratch_path_gives_the_bits_of_the_lds_path():
    T = tile()
    for members in (R.batch_members(T), R.batch_weighted_members(T)):
        g, off = R.concat(members)
        gg = graph_of(g)
        outs = {}
        # the default budget (every graph in LDS), every graph through scratch, graphs of more than T + 1 nodes through scratch
        for budget in (0, 1, (2 * T + 1) * 4 * (T + 1)):
            slab = slab_of(g, R.BATCH_WALK, off)
            assert abi_call(gg, slab, R.BATCH_WALK, G=len(off) - 1, budget=budget) == 0
            assert slab.check({"out": A.E(pred=lambda got: None)}) == [], budget
            outs[budget] = out_of(slab).view(np.uint32)
        assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[(2 * T + 1) * 4 * (T + 1)])
        # without graph_ptr the batch is ONE graph (block diagonal): other tiles, the same bits
        slab = slab_of(g, R.BATCH_WALK)
        assert abi_call(gg, slab, R.BATCH_WALK) == 0
        assert np.array_equal(out_of(slab).view(np.uint32), outs[0])


def test_one_unbatched_graph_of_300_nodes():
    import gnnmp
    g, K, d64, _ = refs()["large"]
    gg = graph_of(g)
    got = host(gnnmp.random_walk_pe(gg, K))
    assert_model(got, "large")
    slab = slab_of(g, K)
    assert abi_call(gg, slab, K, budget=1) == 0                               # and through scratch: 19 tiles in one batch
    assert slab.check({"out": A.E(pred=lambda o: None)}) == []
    assert np.array_equal(out_of(slab).view(np.uint32), got.view(np.uint32))
    unweighted = (g[0], g[1], g[2], None)
    got1 = host(gnnmp.random_walk_pe(graph_of(unweighted), K))
    assert R.within_bar(got1, R.dense64(*unweighted, K)) and not np.array_equal(got1, got)


# ---- the check launch -------------------------------------------------------------------------------------------------------------------
def test_an_edge_between_two_graphs_is_refused():
    import gnnmp
    import torch
    from gnnmp import _lib
    T = tile()
    members = R.batch_weighted_members(T)
    (s, t, n, w), off = R.concat(members)
    t = t.copy()
    e = int(np.flatnonzero(s < off[1])[0])
    t[e] = off[1]                                                              # from the first member into the first node of the second
    g = (s, t, n, w)
    gi = torch.from_numpy(np.repeat(np.arange(1, len(members) + 1), np.diff(off))).cuda()
    gg = graph_of(g, graph_indicator=gi, num_graphs=len(members))
    with pytest.raises(ValueError, match="leaves its graph"):
        gnnmp.random_walk_pe(gg, 4)
    for budget in (None, 1):
        slab = slab_of(g, 4, off)
        assert abi_call(gg, slab, 4, G=len(off) - 1, budget=budget) == _lib.EINVAL
        assert b"leaves its graph" in _lib.load().gnnmp_last_error()
        assert slab.check({}, untouched=True) == []
    # the same edge list is a fine single graph
    assert R.within_bar(host(gnnmp.random_walk_pe(graph_of(g), 4)), R.dense64(*g, 4))


@pytest.mark.parametrize("ib", [8, 4])
def test_a_graph_ptr_that_does_not_ascend_from_0_to_n_is_refused(ib):
    from gnnmp import _lib
    T = tile()
    g, off = R.concat(R.batch_members(T))
    gg = graph_of(g)
    short, long_, late, down = off.copy(), off.copy(), off.copy(), off.copy()
    short[-1] -= 1
    long_[-1] += 1
    late[0] = 1
    down[2], down[3] = off[3], off[2]
    for name, bad in (("short", short), ("long", long_), ("late", late), ("down", down)):
        slab = slab_of(g, 3, bad, ib)
        assert abi_call(gg, slab, 3, G=len(off) - 1, ib=ib) == _lib.EINVAL, name
        assert b"graph_ptr" in _lib.load().gnnmp_last_error(), name
        assert slab.check({}, untouched=True) == [], name


# ---- the memory contract ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("budget", [None, 1], ids=["lds", "scratch"])
def test_writes_all_of_out_and_nothing_else_at_any_alignment(budget):
    """out starts as NaN poison between guard bands: every element is written, no byte outside it (or inside w / graph_ptr) changes, and
    the values do not depend on the alignment of out, w or graph_ptr (4 bytes is all a caller owes)"""
    T = tile()
    g, off = R.concat(R.batch_weighted_members(T))
    gg = graph_of(g)
    K = 5                                                                       # odd: rows of out are 20 bytes, never 16-byte aligned
    d64 = R.dense64(*g, K)
    natural = None
    for ib in (8, 4):
        for what, shifts in (("natural", {}), ("out4", {"out": 4}), ("out8", {"out": 8}), ("w4", {"w": 4}), ("ptr", {"graph_ptr": ib}),
                             ("all", {"out": 4, "w": 4, "graph_ptr": ib})):
            slab = slab_of(g, K, off, ib, shifts=shifts)
            assert np.all(np.isnan(out_of(slab)))
            assert abi_call(gg, slab, K, G=len(off) - 1, ib=ib, budget=budget) == 0, (ib, what)
            assert slab.check({"out": A.E(pred=lambda got: None if not np.isnan(got).any() else "NaN left")}) == [], (ib, what)
            got = out_of(slab)
            if natural is None:
                natural = got
                assert R.within_bar(got, d64)
            assert np.array_equal(got.view(np.uint32), natural.view(np.uint32)), (ib, what)
