"""Device-side edge coalescing and compaction (gnnmp/transform.py, csrc/coalesce.hip) against the numpy restatement of the reference
(tests/transforms_ref.py, itself pinned to the reference's test items in tests/test_transforms_abi.py):

  * index outputs and counts are bit-exact, for every mode, index width and base, at the sizes where the sort and the scan change path;
  * edge data reduced over the coalescing plan is bit-identical to the reference's sequential float32 fold in stably sorted order on
    every output edge whose segment is at most GNNMP_MIN_LONG_ROW long (rows the plan never splits); a longer segment is
    run-to-run deterministic and within 1e-5 relative of the float64 sum;
  * the memory contract of the two writing exports — their device outputs travel in a const host record, so the table of
    tests/abi_cases.py does not reach them — checked here on that module's poisoned, guarded, shifted slab."""
import ctypes
import functools
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_cases as A  # noqa: E402
import transforms_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ("directed", "mirrored", "undirected")
IDX = ((8, 1), (4, 1), (8, 0), (4, 0))                   # (idx_bytes, index_base)
AGGRS = ("+", "mean", "max", "min")
f32 = np.float32


def _constants():
    """the pair sort's per-block tile and the scan's chunk, from the source; the never-split row length from the header"""
    src = open(os.path.join(ROOT, "graphneuralnetworks.jl_amd", "csrc", "sort_scan.hip")).read()
    c = {k: int(re.search(r"constexpr int %s = (\d+);" % k, src).group(1)) for k in ("RS_WT", "RS_WPB", "SC_CHUNK")}
    _, defines = A.parse_header()
    return c["RS_WT"] * c["RS_WPB"], c["SC_CHUNK"], int(defines["GNNMP_MIN_LONG_ROW"])


BLOCK_TILE, SC_CHUNK, MIN_LONG_ROW = _constants()


# ------------------------------------------------------------------------------------------------------------------------------------
# graphs (1-based numpy, like the restatement) and their references, computed once
# ------------------------------------------------------------------------------------------------------------------------------------
def multigraph(E, n, seed):
    """about a third of the edges are copies of other edges, about one in sixteen of the distinct ones is a self loop; shuffled"""
    rng = np.random.default_rng(seed)
    m = E - E // 3
    s = rng.integers(1, n + 1, m)
    t = rng.integers(1, n + 1, m)
    loops = rng.random(m) < 1 / 16
    t[loops] = s[loops]
    dup = rng.integers(0, max(m, 1), E - m)
    s, t = np.concatenate([s, s[dup]]), np.concatenate([t, t[dup]])
    order = rng.permutation(E)
    return s[order].astype(np.int64), t[order].astype(np.int64), n


@functools.lru_cache(maxsize=None)
def index_graphs():
    gs = {"E0": (np.zeros(0, np.int64), np.zeros(0, np.int64), 5)}
    for E in (1, 2, BLOCK_TILE - 1, BLOCK_TILE, BLOCK_TILE + 1, SC_CHUNK - 1, SC_CHUNK, SC_CHUNK + 1):
        gs[f"E{E}"] = multigraph(E, 97 if E > 2 else 3, seed=E)
    gs["E700"] = multigraph(700, 31, seed=81)
    gs["n70000"] = multigraph(300, 70000, seed=11)          # keys need more than 32 bits
    hi = gs["n70000"]
    assert np.any((hi[0] - 1) * 70000 + hi[1] > 2**32)
    v = np.random.default_rng(12).integers(1, 8, 50).astype(np.int64)
    gs["loops"] = (v, v.copy(), 7)                           # all self loops
    gs["one_x40"] = (np.full(40, 3, np.int64), np.full(40, 2, np.int64), 4)
    return gs


@functools.lru_cache(maxsize=None)
def index_ref(name, mode):
    s, t, n = index_graphs()[name]
    if mode == "directed":
        return R.remove_multi_edges(s, t, n)
    return R.to_bidirected(s, t, n) if mode == "mirrored" else R.to_unidirected(s, t, n)


def mk(s, t, n, ib=8, base=1, w=None):
    import torch
    import gnnmp
    dt = torch.int64 if ib == 8 else torch.int32
    return gnnmp.GNNGraph(torch.from_numpy(s - 1 + base).to(dt).cuda(), torch.from_numpy(t - 1 + base).to(dt).cuda(),
                          None if w is None else torch.from_numpy(np.asarray(w, f32)).cuda(), num_nodes=n, index_base=base)


def host(x):
    return x.cpu().numpy()


def edges1(g):
    """(s, t) of a device graph, 1-based int64"""
    return host(g.s).astype(np.int64) + 1 - g.index_base, host(g.t).astype(np.int64) + 1 - g.index_base


# ------------------------------------------------------------------------------------------------------------------------------------
# known answers: the reference's own test items through gnnmp
# ------------------------------------------------------------------------------------------------------------------------------------
def test_reference_items():
    import torch
    import gnnmp
    s, t = np.array([1, 2, 3, 3, 4]), np.array([2, 3, 4, 4, 4])
    w = [1.0, 2.0, 3.0, 4.0, 5.0]
    e = torch.tensor([10.0, 20.0, 30.0, 40.0, 50.0]).cuda()
    g = mk(s, t, 4, w=w)
    g2, e2 = gnnmp.to_bidirected(g, edata=e)
    assert g2.num_nodes == 4 and g2.num_edges == 7
    assert gnnmp.is_bidirected(g2) and not gnnmp.has_multi_edges(g2)
    assert host(g2.s).tolist() == [1, 2, 2, 3, 3, 4, 4] and host(g2.t).tolist() == [2, 1, 3, 2, 4, 3, 4]
    assert host(g2.w).tolist() == [1, 1, 2, 2, 3.5, 3.5, 5]
    assert host(e2).tolist() == [10.0, 10.0, 20.0, 20.0, 35.0, 35.0, 50.0]

    g = mk(np.array([1, 2, 3, 4, 4]), np.array([2, 3, 4, 3, 4]), 4, w=w)
    g2, e2 = gnnmp.to_unidirected(g, edata=e)
    assert g2.num_nodes == 4 and g2.num_edges == 4 and not gnnmp.has_multi_edges(g2)
    assert host(g2.s).tolist() == [1, 2, 3, 4] and host(g2.t).tolist() == [2, 3, 4, 4]
    assert host(g2.w).tolist() == [1, 2, 3.5, 5] and host(e2).tolist() == [10.0, 20.0, 35.0, 50.0]

    assert gnnmp.has_multi_edges(mk(np.array([1, 1, 2, 3]), np.array([2, 2, 2, 4]), 4))
    assert not gnnmp.has_multi_edges(mk(np.array([1, 2, 2, 3]), np.array([2, 1, 2, 4]), 4))
    g = mk(np.array([1, 2, 3]), np.array([2, 3, 2]), 3)
    assert gnnmp.has_isolated_nodes(g) is False and gnnmp.has_isolated_nodes(g, dir="in") is True

    s, t = np.array([1, 1, 2, 3]), np.array([2, 3, 4, 5])
    g = mk(s, t, 5, w=[0.1, 0.2, 0.3, 0.4])
    ed = torch.tensor([97.0, 98.0, 99.0, 100.0]).cuda()
    g2 = gnnmp.remove_edges(g, [1])
    assert g2.num_edges == 3 and host(g2.s).tolist() == [1, 2, 3] and host(g2.t).tolist() == [3, 4, 5]
    g2, ed2 = gnnmp.remove_edges(g, [1, 2, 4], edata=ed)
    assert (host(g2.s).tolist(), host(g2.t).tolist(), host(g2.w).tolist()) == ([2], [4], [float(f32(0.3))])
    assert host(ed2).tolist() == [99.0]
    assert gnnmp.remove_edges(g, 1.0).num_edges == 0 and gnnmp.remove_edges(g, 0.0).num_edges == 4

    # remove_multi_edges (test/transform.jl:303-322): five of twenty edges doubled
    rng = np.random.default_rng(3)
    codes = rng.choice(100, size=20, replace=False)
    s, t = codes // 10 + 1, codes % 10 + 1
    s1, t1 = np.concatenate([s, s[:5]]), np.concatenate([t, t[:5]])
    g1 = mk(s1, t1, 10, w=3 * np.ones(25))
    edata = {"e1": torch.ones(25, 3).cuda(), "e2": 2 * torch.ones(25).cuda()}
    g2, ed2 = gnnmp.remove_multi_edges(g1, edata=edata)
    assert g2.num_edges == 20 and not gnnmp.has_multi_edges(g2) and gnnmp.has_multi_edges(g1)
    assert sorted(zip(*[v.tolist() for v in edges1(g2)])) == sorted(zip(s.tolist(), t.tolist()))
    assert int((host(ed2["e1"]) == 2).all(axis=1).sum()) == 5 and int((host(ed2["e2"]) == 4).sum()) == 5
    assert int((host(g2.w) == 6).sum()) == 5

    # remove_self_loops (test/transform.jl:284-301)
    keep = s != t
    s, t = s[keep], t[keep]
    E = len(s)
    s1, t1 = np.concatenate([s, np.arange(1, 6)]), np.concatenate([t, np.arange(1, 6)])
    g1 = mk(s1, t1, 10, w=3 * np.ones(E + 5))
    g2, ed2 = gnnmp.remove_self_loops(g1, edata={"e1": torch.ones(E + 5, 3).cuda(), "e2": 2 * torch.ones(E + 5).cuda()})
    assert g2.num_edges == E and not gnnmp.has_self_loops(g2)
    assert np.array_equal(edges1(g2)[0], s) and np.array_equal(edges1(g2)[1], t)
    assert tuple(g2.w.shape) == (E,) and tuple(ed2["e1"].shape) == (E, 3) and tuple(ed2["e2"].shape) == (E,)


# ------------------------------------------------------------------------------------------------------------------------------------
# indices, bit-exact against the restatement
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ib,base", IDX)
@pytest.mark.parametrize("mode", MODES)
def test_indices_are_bit_exact(mode, ib, base):
    import torch
    import gnnmp
    for name, (s, t, n) in index_graphs().items():
        ref = index_ref(name, mode)
        g = mk(s, t, n, ib, base)
        g2, co = gnnmp.coalesce_edges(g, mode)
        assert g2.s.dtype == g.s.dtype and g2.index_base == base and g2.num_nodes == n, name
        assert g2.num_edges == len(ref.s) == co.num_edges_out and co.num_edges_in == len(s), name
        s2, t2 = edges1(g2)
        assert np.array_equal(s2, ref.s) and np.array_equal(t2, ref.t), name
        if len(s) == 0:
            assert co.plan is None and tuple(co.reduce(torch.zeros(0, 3).cuda(), "+").shape) == (0, 3)
            continue
        rowptr, col, _ = co.plan.export()
        assert np.array_equal(host(rowptr), np.concatenate([[0], np.cumsum(ref.seg_len)])), name
        assert np.array_equal(host(col), ref.perm % len(s)), name            # a mirrored copy reads the row of the edge it mirrors
        assert not gnnmp.has_multi_edges(g2), name
        assert gnnmp.has_multi_edges(g) == R.has_multi_edges(s, t, n), name
        if mode == "mirrored":
            assert gnnmp.is_bidirected(g2), name


# ------------------------------------------------------------------------------------------------------------------------------------
# edge data over the coalescing plan
# ------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def feature_case(mode):
    """3 000 edges on 40 nodes: segments of one to a dozen copies, all far below the never-split length"""
    s, t, n = multigraph(3000, 40, seed=21)
    rng = np.random.default_rng(22)
    e = {D: rng.standard_normal((3000, D)).astype(f32) for D in (1, 3, 100)}
    refs = {}
    for aggr in AGGRS:
        if mode == "directed":
            refs[aggr] = R.remove_multi_edges(s, t, n, edata=e, aggr=aggr)
        else:
            s2, t2, e2 = s, t, e
            if mode == "mirrored":
                s2, t2, e2 = np.concatenate([s, t]), np.concatenate([t, s]), R.cat_features(e, e)
            else:
                s2, t2 = R.edge_decoding(R.edge_encoding(s, t, n, directed=False)[0], n, directed=False)
            refs[aggr] = R.remove_multi_edges(s2, t2, n, edata=e2, aggr=aggr)
    return s, t, n, e, refs


@pytest.mark.parametrize("mode", MODES)
def test_reduce_is_bit_identical_below_the_split_threshold(mode):
    import torch
    import gnnmp
    s, t, n, e, refs = feature_case(mode)
    g2, co = gnnmp.coalesce_edges(mk(s, t, n), mode)
    assert 1 < refs["+"].seg_len.max() <= MIN_LONG_ROW <= co.plan.long_thresh
    for D, ed in e.items():
        dev = torch.from_numpy(ed).cuda()
        for aggr in AGGRS:
            got = host(co.reduce(dev, aggr))
            assert got.shape == (g2.num_edges, D)
            assert np.array_equal(got, refs[aggr].edata[D]), (mode, D, aggr)
    v = torch.from_numpy(e[1][:, 0].copy()).cuda()                  # a vector [E] comes back as a vector [E2]
    assert np.array_equal(host(co.reduce(v, "+")), refs["+"].edata[1][:, 0])
    x = torch.from_numpy(e[100]).cuda().view(3000, 4, 25)           # trailing dims are flattened and restored
    assert np.array_equal(host(co.reduce(x, "max")).reshape(-1, 100), refs["max"].edata[100])


def test_adds_follow_the_stably_sorted_order():
    """(1e8 + 1) - 1e8 + 1 is 1 in float32 only when the four copies are added left to right in their original order"""
    import torch
    import gnnmp
    s, t = np.array([4, 2, 1, 2, 2, 3, 2]), np.array([1, 3, 1, 3, 3, 3, 3])
    e = np.array([7.0, 1e8, 5.0, 1.0, -1e8, 9.0, 1.0], f32)
    g2, e2 = gnnmp.remove_multi_edges(mk(s, t, 4), edata=torch.from_numpy(e).cuda())
    ref = R.remove_multi_edges(s, t, 4, edata=e)
    assert host(e2).tolist() == ref.edata.tolist() == [5.0, 1.0, 9.0, 7.0]
    # mirrored: the copies of (2, 3) are edges 0 and 2 and the mirrors of edges 1 and 3 — (1e8 - 1e8) + 1 + 1 = 2; those of (3, 2) are
    # edges 1 and 3 and the mirrors of edges 0 and 2 — ((1 + 1) + 1e8) - 1e8 = 0
    s, t = np.array([2, 3, 2, 3]), np.array([3, 2, 3, 2])
    e = np.array([1e8, 1.0, -1e8, 1.0], f32)
    g2, co = gnnmp.coalesce_edges(mk(s, t, 3), "mirrored")
    got = host(co.reduce(torch.from_numpy(e).cuda(), "+"))
    ref = R.remove_multi_edges(np.concatenate([s, t]), np.concatenate([t, s]), 3, edata=np.concatenate([e, e]))
    assert edges1(g2)[0].tolist() == [2, 3] and edges1(g2)[1].tolist() == [3, 2]
    assert got.tolist() == ref.edata.tolist() == [2.0, 0.0]


def test_a_segment_above_the_split_threshold_is_deterministic_and_close():
    import torch
    import gnnmp
    k = MIN_LONG_ROW + 1
    rng = np.random.default_rng(31)
    s = np.concatenate([np.full(k, 5), rng.integers(1, 9, 30)]).astype(np.int64)
    t = np.concatenate([np.full(k, 2), rng.integers(1, 9, 30)]).astype(np.int64)
    order = rng.permutation(len(s))
    s, t = s[order], t[order]
    e = (rng.random((len(s), 3)) + 0.5).astype(f32)                 # uniform in [0.5, 1.5): nothing cancels
    g2, co = gnnmp.coalesce_edges(mk(s, t, 8), "directed")
    dev = torch.from_numpy(e).cuda()
    a, b = host(co.reduce(dev, "+")), host(co.reduce(dev, "+"))
    assert np.array_equal(a, b)
    ref = R.remove_multi_edges(s, t, 8)
    assert ref.seg_len.max() >= k
    exact = np.add.reduceat(e[ref.perm].astype(np.float64), np.concatenate([[0], np.cumsum(ref.seg_len)])[:-1])
    assert np.all(np.abs(a - exact) <= 1e-5 * np.abs(exact))
    short = ref.seg_len <= MIN_LONG_ROW                             # the short segments next to it are still bit-exact
    assert np.array_equal(a[short], R.remove_multi_edges(s, t, 8, edata=e).edata[short])


@pytest.mark.parametrize("mode", MODES)
def test_weights_and_dict_edata_travel_together(mode):
    import torch
    import gnnmp
    s, t, n = multigraph(500, 12, seed=41)
    rng = np.random.default_rng(42)
    w = rng.random(500).astype(f32)
    ed = {"a": rng.standard_normal((500, 3)).astype(f32), "b": rng.standard_normal(500).astype(f32)}
    dev = {k: torch.from_numpy(v).cuda() for k, v in ed.items()}
    g = mk(s, t, n, w=w)
    if mode == "directed":
        for aggr in ("max", "+"):
            g2, ed2 = gnnmp.remove_multi_edges(g, aggr=aggr, edata=dev)
            ref = R.remove_multi_edges(s, t, n, w, ed, aggr=aggr)
            assert set(ed2) == {"a", "b"} and np.array_equal(host(g2.w), ref.w)
            assert all(np.array_equal(host(ed2[k]), ref.edata[k]) for k in ed)
        assert isinstance(gnnmp.remove_multi_edges(g), gnnmp.GNNGraph)
        return
    f, rf = (gnnmp.to_bidirected, R.to_bidirected) if mode == "mirrored" else (gnnmp.to_unidirected, R.to_unidirected)
    g2, ed2 = f(g, edata=dev)
    ref = rf(s, t, n, w, ed)
    assert np.array_equal(edges1(g2)[0], ref.s) and np.array_equal(host(g2.w), ref.w)
    assert all(np.array_equal(host(ed2[k]), ref.edata[k]) for k in ed)
    g3 = f(mk(s, t, n))
    assert isinstance(g3, gnnmp.GNNGraph) and g3.w is None and g3.num_edges == g2.num_edges


def test_error_types():
    import torch
    import gnnmp
    s, t, n = multigraph(50, 6, seed=51)
    g = mk(s, t, n)
    with pytest.raises(ValueError):
        gnnmp.coalesce_edges(g, "both")
    with pytest.raises(ValueError):
        gnnmp.remove_multi_edges(g, aggr="prod")
    g2, co = gnnmp.coalesce_edges(g)
    with pytest.raises(ValueError):
        co.reduce(torch.zeros(50, 2).cuda(), "*")
    with pytest.raises(AssertionError):
        co.reduce(torch.zeros(49, 2).cuda(), "+")
    with pytest.raises(AssertionError):
        gnnmp.to_bidirected(g, edata=torch.zeros(51).cuda())
    with pytest.raises(AssertionError):
        gnnmp.remove_self_loops(g, edata={"a": torch.zeros(3, 2).cuda()})
    with pytest.raises(IndexError):
        gnnmp.remove_edges(g, [1, 51])
    with pytest.raises(IndexError):
        gnnmp.remove_edges(g, [0])
    with pytest.raises(ValueError):
        gnnmp.remove_edges(g, 1.5)
    with pytest.raises(ValueError):
        gnnmp.has_isolated_nodes(g, dir="both")


# ------------------------------------------------------------------------------------------------------------------------------------
# remove_self_loops / remove_edges
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ib,base", IDX)
def test_compaction_is_exact(ib, base):
    import torch
    import gnnmp
    rng = np.random.default_rng(61)
    for E in (1, 2, 700, SC_CHUNK, SC_CHUNK + 1):
        s, t, n = multigraph(E, 23, seed=60 + E)
        w = rng.random(E).astype(f32)
        ed = {"a": rng.standard_normal((E, 3)).astype(f32), "b": np.arange(E, dtype=f32)}
        dev = {k: torch.from_numpy(v).cuda() for k, v in ed.items()}
        g = mk(s, t, n, ib, base, w=w)

        def same(out, ref):
            g2, ed2 = out
            rs, rt, rw, re_, kept = ref
            assert g2.num_edges == len(rs) and g2.s.dtype == g.s.dtype and g2.index_base == base
            s2, t2 = edges1(g2)
            assert np.array_equal(s2, rs) and np.array_equal(t2, rt) and np.array_equal(host(g2.w), rw)
            assert all(np.array_equal(host(ed2[k]), re_[k]) for k in ed)
            assert np.array_equal(host(ed2["b"]), kept.astype(f32))               # eid gathered the kept rows

        same(gnnmp.remove_self_loops(g, edata=dev), R.remove_self_loops(s, t, w, ed))
        lists = [rng.integers(1, E + 1, max(E // 3, 1)), np.zeros(0, np.int64), np.arange(1, E + 1),
                 np.repeat(rng.integers(1, E + 1, 3), 4)]                         # with repeats, empty, full, one position many times
        for rm in lists:
            dt = torch.int64 if ib == 8 else torch.int32
            same(gnnmp.remove_edges(g, torch.from_numpy(rm - 1 + base).to(dt).cuda(), edata=dev), R.remove_edges(s, t, rm, w, ed))
        same(gnnmp.remove_edges(g, [base], edata=dev), R.remove_edges(s, t, [1], w, ed))          # a plain Python list


def test_random_removal():
    import torch
    import gnnmp
    s, t, n = multigraph(4096, 50, seed=71)
    g = mk(s, t, n, w=np.arange(4096, dtype=f32))
    pos = torch.arange(4096, dtype=torch.float32).cuda()
    g0 = gnnmp.remove_edges(g, 0.0, seed=5)
    assert g0.num_edges == 4096 and np.array_equal(edges1(g0)[0], s) and np.array_equal(edges1(g0)[1], t)
    assert gnnmp.remove_edges(g, 1.0, seed=5).num_edges == 0
    ga, ea = gnnmp.remove_edges(g, 0.5, edata=pos, seed=123)
    gb, eb = gnnmp.remove_edges(g, 0.5, edata=pos, seed=123)
    assert np.array_equal(host(ga.s), host(gb.s)) and np.array_equal(host(ga.t), host(gb.t)) and np.array_equal(host(ea), host(eb))
    # six binomial standard deviations: sigma = sqrt(4096 / 4) = 32
    assert abs(ga.num_edges - 2048) <= 192
    kept = host(ea).astype(np.int64)
    assert np.all(np.diff(kept) > 0)                                               # stable: the kept positions ascend
    assert np.array_equal(edges1(ga)[0], s[kept]) and np.array_equal(edges1(ga)[1], t[kept]) and np.array_equal(host(ga.w), kept.astype(f32))
    gc = gnnmp.remove_edges(g, 0.5, seed=124)
    assert not (gc.num_edges == ga.num_edges and np.array_equal(host(gc.s), host(ga.s)))      # another seed, another graph


# ------------------------------------------------------------------------------------------------------------------------------------
# the memory contract of the two writing exports, on the guarded slab of tests/abi_cases.py
# ------------------------------------------------------------------------------------------------------------------------------------
def _untouched_tail(slab, name, count):
    """elements [count, capacity) of an output still carry the poison"""
    a = slab.arrs[name]
    after = slab.t.cpu().numpy()
    lo = a.off + count * a.dtype.itemsize
    return np.array_equal(after[lo:a.off + a.nbytes], slab.before[lo:a.off + a.nbytes])


def _shift_sets(names, ib):
    yield "natural", {}
    yield "all", {k: ib for k in names}                    # the smallest alignment a caller may pass: one element (4 bytes for Int32)
    for k in names:
        yield k, {k: ib}


@pytest.mark.parametrize("ib,base", IDX)
@pytest.mark.parametrize("mode", MODES)
def test_coalesce_writes_its_outputs_and_nothing_else(mode, ib, base):
    from gnnmp import _lib
    lib = _lib.load()
    dt = np.int64 if ib == 8 else np.int32
    for name in ("E700", "one_x40"):
        s, t, n = index_graphs()[name]
        ref = index_ref(name, mode)
        E = len(s)
        Ev = 2 * E if mode == "mirrored" else E
        k = len(ref.s)
        expected = {"s_out": A.E((ref.s - 1 + base).astype(dt), "exact", prefix=k), "t_out": A.E((ref.t - 1 + base).astype(dt), "exact", prefix=k),
                    "colptr": A.E((np.concatenate([[0], np.cumsum(ref.seg_len)]) + base).astype(dt), "exact", prefix=k + 1),
                    "rowval": A.E((ref.perm % E + base).astype(dt), "exact")}
        for what, shifts in _shift_sets(("s", "t", "s_out", "t_out", "colptr", "rowval"), ib):
            slab = A.Slab([A.Arr("s", "in", (s - 1 + base).astype(dt)), A.Arr("t", "in", (t - 1 + base).astype(dt)),
                           A.Arr("s_out", "out", shape=Ev, dtype=dt), A.Arr("t_out", "out", shape=Ev, dtype=dt),
                           A.Arr("colptr", "out", shape=Ev + 1, dtype=dt), A.Arr("rowval", "out", shape=Ev, dtype=dt)], shifts=shifts)
            job = _lib.CoalesceJob(slab.ptr("s"), slab.ptr("t"), ib, base, E, n, MODES.index(mode), slab.ptr("s_out"), slab.ptr("t_out"),
                                   slab.ptr("colptr"), slab.ptr("rowval"))
            total = ctypes.c_int64(-1)
            rc = lib.gnnmp_coalesce_edges(ctypes.byref(job), ctypes.byref(total), _lib.stream_ptr())
            assert rc == 0 and total.value == k, (name, what, rc, lib.gnnmp_last_error())
            assert slab.check(expected) == [], (name, what)        # inputs bit for bit, [0, total) written and right, guards intact
            assert _untouched_tail(slab, "s_out", k) and _untouched_tail(slab, "t_out", k) and _untouched_tail(slab, "colptr", k + 1), (name, what)
    # a refused call (an index outside the nodes, found on the device) leaves every byte as it was
    s, t, n = index_graphs()["E700"]
    slab = A.Slab([A.Arr("s", "in", (s - 1 + base).astype(dt)), A.Arr("t", "in", (t - 1 + base).astype(dt)),
                   A.Arr("s_out", "out", shape=1400, dtype=dt), A.Arr("t_out", "out", shape=1400, dtype=dt),
                   A.Arr("colptr", "out", shape=1401, dtype=dt), A.Arr("rowval", "out", shape=1400, dtype=dt)])
    job = _lib.CoalesceJob(slab.ptr("s"), slab.ptr("t"), ib, base, 700, 30, MODES.index(mode), slab.ptr("s_out"), slab.ptr("t_out"),
                           slab.ptr("colptr"), slab.ptr("rowval"))
    total = ctypes.c_int64(-1)
    assert lib.gnnmp_coalesce_edges(ctypes.byref(job), ctypes.byref(total), _lib.stream_ptr()) == _lib.EBOUNDS and total.value == 0
    assert slab.check({}, untouched=True) == []


@pytest.mark.parametrize("ib,base", IDX)
@pytest.mark.parametrize("rule", (0, 1, 2))
def test_compact_writes_its_outputs_and_nothing_else(rule, ib, base):
    from gnnmp import _lib
    lib = _lib.load()
    dt = np.int64 if ib == 8 else np.int32
    E = 700
    s, t, n = multigraph(E, 31, seed=82)
    rng = np.random.default_rng(83)
    w = rng.random(E).astype(f32)
    rm = rng.integers(1, E + 1, 200)
    arrs = lambda: [A.Arr("s", "in", (s - 1 + base).astype(dt)), A.Arr("t", "in", (t - 1 + base).astype(dt)), A.Arr("w", "in", w),
                    A.Arr("remove", "in", (rm - 1 + base).astype(dt)), A.Arr("s_out", "out", shape=E, dtype=dt),
                    A.Arr("t_out", "out", shape=E, dtype=dt), A.Arr("w_out", "out", shape=E), A.Arr("eid_out", "out", shape=E, dtype=dt)]
    job_of = lambda slab, n_remove=200: _lib.CompactJob(slab.ptr("s"), slab.ptr("t"), slab.ptr("w"), ib, base, E, rule, slab.ptr("remove"),
                                                        n_remove, 0.5, 77, slab.ptr("s_out"), slab.ptr("t_out"), slab.ptr("w_out"),
                                                        slab.ptr("eid_out"))
    kept = None
    if rule == 0:
        kept = R.remove_self_loops(s, t)[4]
    elif rule == 1:
        kept = R.remove_edges(s, t, rm)[4]
    for what, shifts in _shift_sets(("s", "t", "remove", "s_out", "t_out", "eid_out"), ib):
        slab = A.Slab(arrs(), shifts=shifts)
        total = ctypes.c_int64(-1)
        rc = lib.gnnmp_compact_edges(ctypes.byref(job_of(slab)), ctypes.byref(total), _lib.stream_ptr())
        assert rc == 0, (what, lib.gnnmp_last_error())
        k = total.value
        if kept is None:                                      # the random rule: the first run's kept positions are every later run's
            kept = slab.get(slab.t.cpu().numpy(), "eid_out")[:k].astype(np.int64) - base
            assert abs(k - E // 2) <= 6 * np.sqrt(E / 4) and np.all(np.diff(kept) > 0) and kept.min() >= 0 and kept.max() < E
        assert k == len(kept), what
        expected = {"s_out": A.E((s[kept] - 1 + base).astype(dt), "exact", prefix=k), "t_out": A.E((t[kept] - 1 + base).astype(dt), "exact", prefix=k),
                    "w_out": A.E(w[kept], "exact", prefix=k), "eid_out": A.E((kept + base).astype(dt), "exact", prefix=k)}
        assert slab.check(expected) == [], what
        assert all(_untouched_tail(slab, o, k) for o in ("s_out", "t_out", "w_out", "eid_out")), what
    if rule == 1:                                             # a listed position outside the edges: refused, nothing written
        bad = rm.copy()
        bad[17] = E + 1
        slab = A.Slab(arrs())
        slab.reload({"remove": (bad - 1 + base).astype(dt)})
        total = ctypes.c_int64(-1)
        assert lib.gnnmp_compact_edges(ctypes.byref(job_of(slab)), ctypes.byref(total), _lib.stream_ptr()) == _lib.EBOUNDS and total.value == 0
        assert slab.check({}, untouched=True) == []
