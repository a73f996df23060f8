"""Heterographs on the device: hetero_rows_kernel (csrc/hetero.hip) through gnnmp_hetero_propagate_f32, its memory contract and its
capture into a HIP graph, GNNHeteroGraph, and HeteroGraphConv's two paths.

Bars: for + / max / min relations the kernel's result is BIT-IDENTICAL to the ordered float32 restatement (tests/hetero_ref.py: adds in
original edge order, fold in relation order); a mean relation is bit-identical to gnnmp.propagate on that relation, whose finish it
shares; everything is within 1e-5 of the float64 restatement by the comparison of the ABI tests (abi_cases.compare: norm-wise and
element-wise against the reference's scale, identities of empty rows equal)."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_cases as A  # noqa: E402
import hetero_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

OPS = ("+", "mean", "max", "min")
CODE = {"+": 0, "mean": 1, "max": 2, "min": 3}


@pytest.fixture(scope="module")
def gm():
    import torch
    assert torch.cuda.is_available()
    import gnnmp
    return gnnmp


@pytest.fixture(scope="module")
def cap():
    from gnnmp import _lib
    return _lib.HETERO_MAX_REL


def close64(got, ref, what):
    msg = A.compare(np.asarray(got), np.asarray(ref), A.E(tol="rel"))
    assert msg is None, f"{what}: {msg}"


def close64_layer(got, ref, what):
    """a layer output: a max / min aggregate of an empty row is ∓Inf (NNlib.scatter's identity), and its dense product is Inf or NaN
    depending on the order of the sum — non-finite in the same places, the finite rest by the usual comparison"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    fin = np.isfinite(ref)
    assert np.array_equal(np.isfinite(got), fin), f"{what}: non-finite entries (empty rows under max / min) in other places than the reference's"
    close64(np.where(fin, got, 0.0).astype(np.float32), np.where(fin, ref, 0.0), what)


def same_bits(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, what
    assert np.array_equal(got, want, equal_nan=True), \
        f"{what}: {int((~((got == want) | ((got != got) & (want != want)))).sum())} of {got.size} elements differ from the ordered float32 reference"


# ------------------------------------------------------------------------------------------------------------------------------------
# a synthetic destination type: R relations of different source counts (1 included), one without edges (R > 2: relation 1, a weighted
# mean, whose identity 0 leaves the other terms visible), rows that are empty in every relation (i % 5 == 3), operators + / mean / max /
# min in turn, every second relation weighted
# ------------------------------------------------------------------------------------------------------------------------------------
N_SRC = (13, 1, 40, 5)


def make_dst(rng, name, n_dst, R, D):
    """[(edge_t, s0, t0, n_src, x, w | None, aggr)] — 0-based indices"""
    rows = np.array([i for i in range(n_dst) if i % 5 != 3] or [0])
    rels = []
    for r in range(R):
        n_src = N_SRC[r % 4] + r // 4
        E = 0 if (r == 1 and R > 2) else 3 * n_dst + r
        s0, t0 = rng.integers(0, n_src, E), rows[rng.integers(0, len(rows), E)]
        x = rng.uniform(-1, 1, (n_src, D)).astype(np.float32)
        w = rng.uniform(0.5, 1.5, E).astype(np.float32) if r % 2 else None
        rels.append(((f"{name}_s{r}", "r", name), s0, t0, n_src, x, w, OPS[r % 4]))
    return rels


def build_graph(gm, dsts, idx=np.int64, base=1):
    """dsts: {name: (n_dst, rels)} -> (graph, x by node type on the device, aggr / edge_weight dicts)"""
    import torch
    data, num_nodes, x, aggr, ew = {}, {}, {}, {}, {}
    for name, (n_dst, rels) in dsts.items():
        num_nodes[name] = n_dst
        for et, s0, t0, n_src, xs, w, op in rels:
            data[et] = (torch.from_numpy((s0 + base).astype(idx)).cuda(), torch.from_numpy((t0 + base).astype(idx)).cuda())
            num_nodes[et[0]] = n_src
            x[et[0]] = torch.from_numpy(xs).cuda()
            aggr[et] = op
            if w is not None:
                ew[et] = torch.from_numpy(w).cuda()
    g = gm.GNNHeteroGraph(data, num_nodes=num_nodes, index_base=base)
    return g, x, aggr, ew


def expected(gm, g, x, rels, n_dst, combine):
    """(the bits the kernel owes, the float64 value): restatement per relation — a mean relation's float32 term is gnnmp.propagate's"""
    terms32 = []
    for et, s0, t0, n_src, xs, w, op in rels:
        if op == "mean":
            sub = gm.edge_type_subgraph(g, et)
            if w is None:
                m = gm.propagate(gm.copy_xj, sub, "mean", xj=x[et[0]])
            else:
                m = gm.propagate(gm.e_mul_xj, sub, "mean", xj=x[et[0]], e=_dev(w))
            assert m.shape[0] == n_dst
            terms32.append(m.cpu().numpy())
        else:
            terms32.append(R.propagate_ref(s0, t0, n_dst, xs, w, op, np.float32))
    ref64 = R.hetero_ref([(s0, t0, xs, w, op) for _, s0, t0, _, xs, w, op in rels], n_dst, combine, np.float64)
    return R.fold_ref(terms32, combine), ref64


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def spy(monkeypatch, lib, *names):
    """count the calls of the named exports"""
    counts = {n: 0 for n in names}
    for n in names:
        real = getattr(lib, n)

        def wrapped(*a, _real=real, _n=n):
            counts[_n] += 1
            return _real(*a)
        monkeypatch.setattr(lib, n, wrapped)
    return counts


# ------------------------------------------------------------------------------------------------------------------------------------
# the kernel
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_dst", [1, 31, 33, 300])
@pytest.mark.parametrize("R_", [1, 2, "cap"])
@pytest.mark.parametrize("D", [1, 3, 4, 100, 260])
def test_one_launch_matches_the_ordered_restatement(gm, cap, monkeypatch, D, R_, n_dst):
    from gnnmp import _lib
    Rn = cap if R_ == "cap" else R_
    rng = np.random.default_rng([D, Rn, n_dst])
    rels = make_dst(rng, "d", n_dst, Rn, D)
    combine = ("+", "max", "min")[(D + Rn + n_dst) % 3]
    g, x, aggr, ew = build_graph(gm, {"d": (n_dst, rels)})
    want32, ref64 = expected(gm, g, x, rels, n_dst, combine)
    counts = spy(monkeypatch, _lib.load(), "gnnmp_hetero_propagate_f32", "gnnmp_propagate_f32")
    y = gm.hetero_propagate(g, x, aggr=aggr, combine=combine, edge_weight=ew)
    assert counts == {"gnnmp_hetero_propagate_f32": 1, "gnnmp_propagate_f32": 0}
    assert list(y) == ["d"]
    got = y["d"].cpu().numpy()
    same_bits(got, want32, f"D={D} R={Rn} n_dst={n_dst} combine={combine}")
    close64(got, ref64, "against float64")


@pytest.mark.parametrize("with_root", [False, True])
def test_two_destination_types_of_different_sizes_in_one_launch(gm, monkeypatch, with_root):
    from gnnmp import _lib
    import torch
    D = 100
    rng = np.random.default_rng(7)
    dsts = {"a": (33, make_dst(rng, "a", 33, 3, D)), "b": (300, make_dst(rng, "b", 300, 4, D))}
    g, x, aggr, ew = build_graph(gm, dsts)
    root = {k: rng.uniform(-1, 1, (n, D)).astype(np.float32) for k, (n, _) in dsts.items()} if with_root else None
    counts = spy(monkeypatch, _lib.load(), "gnnmp_hetero_propagate_f32")
    y = gm.hetero_propagate(g, x, aggr=aggr, combine="+", edge_weight=ew,
                            root=None if root is None else {k: torch.from_numpy(v).cuda() for k, v in root.items()})
    assert counts["gnnmp_hetero_propagate_f32"] == 1 and list(y) == ["a", "b"]
    for k, (n, rels) in dsts.items():
        want32, ref64 = expected(gm, g, x, rels, n, "+")
        if with_root:
            want32 = R.fold_ref([root[k]] + [expected(gm, g, x, [rel], n, "+")[0] for rel in rels], "+")      # the root enters the fold first
            ref64 = R.hetero_ref([(s0, t0, xs, w, op) for _, s0, t0, _, xs, w, op in rels], n, "+", np.float64, root=root[k])
        same_bits(y[k].cpu().numpy(), want32, f"destination type {k}")
        close64(y[k].cpu().numpy(), ref64, f"destination type {k} against float64")


@pytest.mark.parametrize("idx,base", [(np.int64, 1), (np.int32, 1), (np.int64, 0), (np.int32, 0)])
def test_index_widths_and_bases(gm, idx, base):
    rng = np.random.default_rng(11)
    rels = make_dst(rng, "d", 33, 4, 4)
    g, x, aggr, ew = build_graph(gm, {"d": (33, rels)}, idx, base)
    assert g.idx_bytes == np.dtype(idx).itemsize and g.index_base == base
    want32, ref64 = expected(gm, g, x, rels, 33, "+")
    got = gm.hetero_propagate(g, x, aggr=aggr, edge_weight=ew)["d"].cpu().numpy()
    same_bits(got, want32, f"{idx.__name__} base {base}")
    close64(got, ref64, "against float64")


def test_a_row_of_five_times_the_split_threshold(gm, monkeypatch):
    """the kernel walks a split row whole, in edge order: the bits of the sequential loop; hetero_propagate sends the graph to the composition"""
    import torch
    from gnnmp import _lib, hetero
    D, n_dst = 100, 33
    rng = np.random.default_rng(13)
    rels = make_dst(rng, "d", n_dst, 2, D)
    thr = _lib.LONG_ROW // 8                                 # GNNMP_MIN_LONG_ROW: the threshold of a small plan — read back below
    et, s0, t0, n_src, xs, w, _ = rels[1]
    hub = 5 * thr - int((t0 == 7).sum())
    s0, t0 = np.concatenate([s0, rng.integers(0, n_src, hub)]), np.concatenate([t0, np.full(hub, 7)])
    perm = rng.permutation(len(s0))
    s0, t0 = s0[perm], t0[perm]
    rels[1] = (et, s0, t0, n_src, xs, rng.uniform(0.5, 1.5, len(s0)).astype(np.float32), "+")
    rels[0] = rels[0][:6] + ("max",)
    g, x, aggr, ew = build_graph(gm, {"d": (n_dst, rels)})
    p = g.plan(et)
    assert p.long_thresh == thr and p.n_long == 1 and int((t0 == 7).sum()) == 5 * p.long_thresh
    want32, ref64 = expected(gm, g, x, rels, n_dst, "+")
    out = torch.empty((n_dst, D), dtype=torch.float32, device="cuda")
    recs = [(g.plan(e), x[e[0]], ew.get(e), CODE[op]) for e, _, _, _, _, _, op in rels]
    hetero._hetero_call([(out, n_dst, 0, recs)], D)
    same_bits(out.cpu().numpy(), want32, "the kernel on a split row")
    counts = spy(monkeypatch, _lib.load(), "gnnmp_hetero_propagate_f32", "gnnmp_propagate_f32")
    y = gm.hetero_propagate(g, x, aggr=aggr, combine="+", edge_weight=ew)["d"].cpu().numpy()
    assert counts == {"gnnmp_hetero_propagate_f32": 1, "gnnmp_propagate_f32": 2}      # propagate per relation + the combiner
    close64(y, ref64, "the composition on a split row")
    short = np.arange(n_dst) != 7
    same_bits(y[short], want32[short], "the composition on the rows that are not split")


def test_more_relations_than_the_cap_take_the_composition(gm, cap, monkeypatch):
    from gnnmp import _lib
    rng = np.random.default_rng(17)
    rels = make_dst(rng, "d", 31, cap + 3, 4)
    g, x, aggr, ew = build_graph(gm, {"d": (31, rels)})
    want32, ref64 = expected(gm, g, x, rels, 31, "max")
    counts = spy(monkeypatch, _lib.load(), "gnnmp_hetero_propagate_f32", "gnnmp_propagate_f32")
    y = gm.hetero_propagate(g, x, aggr=aggr, combine="max", edge_weight=ew)["d"].cpu().numpy()
    assert counts == {"gnnmp_hetero_propagate_f32": 2, "gnnmp_propagate_f32": cap + 3}     # the fold of cap + 3 terms: two calls
    same_bits(y, want32, "composition over the cap")
    close64(y, ref64, "against float64")


def test_the_knob_forces_the_composition(gm, monkeypatch):
    from gnnmp import _lib
    rng = np.random.default_rng(19)
    rels = make_dst(rng, "d", 33, 3, 100)
    g, x, aggr, ew = build_graph(gm, {"d": (33, rels)})
    one = gm.hetero_propagate(g, x, aggr=aggr, edge_weight=ew)["d"].cpu().numpy()
    counts = spy(monkeypatch, _lib.load(), "gnnmp_hetero_propagate_f32", "gnnmp_propagate_f32")
    with _lib.tuned(_lib.Knob.HETERO, -1):
        two = gm.hetero_propagate(g, x, aggr=aggr, edge_weight=ew)["d"].cpu().numpy()
    assert counts == {"gnnmp_hetero_propagate_f32": 1, "gnnmp_propagate_f32": 3}
    same_bits(two, one, "the composition against the one-launch kernel (no split rows: the same bits)")


def test_a_plan_of_another_height_and_a_bad_operator_are_refused(gm):
    import torch
    from gnnmp import _lib, hetero
    rng = np.random.default_rng(23)
    rels = make_dst(rng, "d", 31, 1, 4)
    g, x, _, _ = build_graph(gm, {"d": (31, rels)})
    et = rels[0][0]
    out = torch.full((40, 4), 7.0, device="cuda")
    with pytest.raises(_lib.GnnmpError) as e:
        hetero._hetero_call([(out, 40, 0, [(g.plan(et), x[et[0]], None, 0)])], 4)
    assert e.value.status == _lib.EINVAL and "destinations" in str(e.value)
    with pytest.raises(_lib.GnnmpError) as e:
        hetero._hetero_call([(out, 31, 0, [(g.plan(et), x[et[0]], None, 9)])], 4)
    assert e.value.status == _lib.EINVAL and "bad aggr" in str(e.value)
    assert bool((out == 7.0).all())


# ------------------------------------------------------------------------------------------------------------------------------------
# the memory contract and capture: every array of the call inside abi_cases' poisoned slab
# ------------------------------------------------------------------------------------------------------------------------------------
class SlabCall:
    """two destination types (33 and 300 rows), an identity relation (root), weighted and unweighted relations, all four operators"""

    def __init__(self, gm, D, seed=29, shift=0):
        rng = np.random.default_rng(seed)
        self.D = D
        self.dsts = {"a": (33, make_dst(rng, "a", 33, 3, D)), "b": (300, make_dst(rng, "b", 300, 4, D))}
        self.g, self.x, _, _ = build_graph(gm, self.dsts)
        self.root = rng.uniform(-1, 1, (33, D)).astype(np.float32)
        arrs = [A.Arr("out_a", "out", shape=(33, D)), A.Arr("out_b", "out", shape=(300, D)), A.Arr("root_a", "in", self.root)]
        for name, (_, rels) in self.dsts.items():
            for r, (_, _, _, _, xs, w, _) in enumerate(rels):
                arrs.append(A.Arr(f"x_{name}{r}", "in", xs))
                if w is not None and len(w):
                    arrs.append(A.Arr(f"w_{name}{r}", "in", w))
        self.slab = A.Slab(arrs, "cuda", {a.name: shift for a in arrs})
        self.keep = []

    def tables(self, combine=0, bad_aggr=None):
        from gnnmp import _lib
        dsts = (_lib.HeteroDst * 2)()
        for d, (name, (n, rels)) in zip(dsts, self.dsts.items()):
            ident = 1 if name == "a" else 0
            tab = (_lib.HeteroRel * (len(rels) + ident))()
            if ident:
                tab[0].plan, tab[0].x, tab[0].w, tab[0].aggr = None, self.slab.ptr("root_a"), None, 0
            for r, (et, _, _, _, _, w, op) in enumerate(rels):
                q = tab[r + ident]
                q.plan, q.x, q.aggr = self.g.plan(et).handle, self.slab.ptr(f"x_{name}{r}"), CODE[op] if bad_aggr is None else bad_aggr
                q.w = self.slab.ptr(f"w_{name}{r}") if (w is not None and len(w)) else None
            self.keep.append(tab)
            d.out, d.n_dst, d.combine, d.n_rel, d.rels = self.slab.ptr(f"out_{name}"), n, combine, len(tab), tab
        return dsts

    def reference(self, gm, data=None):
        """{out: E(exact float32 bits)} for the arrays as they are in the slab (data: {array name: new values})"""
        data = data or {}
        ref = {}
        for name, (n, rels) in self.dsts.items():
            terms = [data.get("root_a", self.root)] if name == "a" else []
            for r, (et, s0, t0, _, xs, w, op) in enumerate(rels):
                xs, w = data.get(f"x_{name}{r}", xs), (data.get(f"w_{name}{r}", w) if w is not None else None)
                if op == "mean":
                    sub = gm.edge_type_subgraph(self.g, et)
                    m = gm.propagate(gm.copy_xj, sub, "mean", xj=_dev(xs)) if w is None else \
                        gm.propagate(gm.e_mul_xj, sub, "mean", xj=_dev(xs), e=_dev(w))
                    terms.append(m.cpu().numpy())
                else:
                    terms.append(R.propagate_ref(s0, t0, n, xs, w, op, np.float32))
            ref[f"out_{name}"] = A.E(R.fold_ref(terms, "+"), "exact")
        return ref


@pytest.mark.parametrize("D,shift", [(100, 0), (3, 0), (260, 0), (100, 4), (4, 4), (6, 8)])
def test_writes_all_of_its_output_and_nothing_else(gm, D, shift):
    """every element of both outputs written, no stray store, the inputs untouched — at natural alignment and with every pointer shifted
    to 4-byte (8-byte) alignment, where the 16-byte lanes must give way to narrower ones"""
    import torch
    from gnnmp import _lib
    c = SlabCall(gm, D, shift=shift)
    rc = _lib.load().gnnmp_hetero_propagate_f32(c.tables(), 2, D, None)
    torch.cuda.synchronize()
    assert rc == _lib.OK, _lib.load().gnnmp_last_error()
    problems = c.slab.check(c.reference(gm))
    assert not problems, "\n".join(problems)


def test_a_refused_call_leaves_the_slab_untouched(gm, cap):
    import torch
    from gnnmp import _lib
    lib = _lib.load()
    c = SlabCall(gm, 100)
    assert lib.gnnmp_hetero_propagate_f32(c.tables(combine=1), 2, 100, None) == _lib.EINVAL          # mean is no fold
    assert lib.gnnmp_hetero_propagate_f32(c.tables(bad_aggr=5), 2, 100, None) == _lib.EINVAL
    assert lib.gnnmp_hetero_propagate_f32(c.tables(), 2, 0, None) == _lib.EINVAL
    wide = c.tables()
    wide[1].n_rel = cap                                                                             # 4 + cap relations announced
    assert lib.gnnmp_hetero_propagate_f32(wide, 2, 100, None) == _lib.EUNSUPPORTED
    torch.cuda.synchronize()
    problems = c.slab.check({}, untouched=True)
    assert not problems, "\n".join(problems)


def test_capture_replay_new_values_and_back_to_back(gm):
    """recorded on ONE stream (no parallel branches) without an eager call first — the export uses no plan scratch; nothing runs while it
    is recorded; a replay gives the eager bits; new values at the same addresses give the new reference; two replays back to back agree"""
    import torch
    from gnnmp import _lib
    lib = _lib.load()
    D = 100
    c = SlabCall(gm, D)
    ref0 = c.reference(gm)
    dsts = c.tables()
    side = torch.cuda.Stream()
    sp = ctypes.c_void_p(side.cuda_stream)
    torch.cuda.synchronize()

    graph = torch.cuda.CUDAGraph()
    err = []
    with torch.cuda.stream(side):
        graph.capture_begin(capture_error_mode="thread_local")
        try:
            rc = lib.gnnmp_hetero_propagate_f32(dsts, 2, D, sp)
        finally:
            graph.capture_end()
            torch.cuda.synchronize()
    assert rc == _lib.OK and not err, lib.gnnmp_last_error()
    problems = c.slab.check({}, untouched=True)
    assert not problems, "work ran while the call was being recorded: " + "\n".join(problems)

    graph.replay()
    torch.cuda.synchronize()
    problems = c.slab.check(ref0)
    assert not problems, "replay 1: " + "\n".join(problems)
    first = c.slab.outputs()

    c.slab.reload()
    assert lib.gnnmp_hetero_propagate_f32(dsts, 2, D, sp) == _lib.OK                                 # the eager call, same stream
    torch.cuda.synchronize()
    eager = c.slab.outputs()
    assert all(np.array_equal(first[k], eager[k]) for k in eager), "replay 1 differs from the eager call"

    rng = np.random.default_rng(31)
    new = {a.name: (rng.uniform(0.5, 1.5, a.shape) if a.name.startswith("w_") else rng.uniform(-1, 1, a.shape)).astype(np.float32)
           for a in c.slab.arrs.values() if a.role == "in"}
    ref1 = c.reference(gm, new)
    c.slab.reload(new)
    graph.replay()
    torch.cuda.synchronize()
    problems = c.slab.check(ref1)
    assert not problems, "replay 2, new values in the same buffers: " + "\n".join(problems)
    second = c.slab.outputs()

    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    last = c.slab.outputs()
    assert all(np.array_equal(last[k], second[k]) for k in second), "two replays back to back differ from replay 2"
    del graph


# ------------------------------------------------------------------------------------------------------------------------------------
# the graph
# ------------------------------------------------------------------------------------------------------------------------------------
def test_graph_counts_types_queries_and_checks(gm):
    import torch
    rng = np.random.default_rng(37)
    ets = [("user", "rates", "item"), ("item", "rated_by", "user"), ("user", "follows", "user")]
    n = {"user": 9, "item": 14}
    coo = {et: (rng.integers(1, n[et[0]] + 1, 25), rng.integers(1, n[et[2]] + 1, 25)) for et in ets}
    w = rng.uniform(0, 1, 25).astype(np.float32)
    data = {et: (coo[et] + ((w,) if et == ets[0] else ())) for et in ets}
    g = gm.GNNHeteroGraph(data, num_nodes=n)
    assert g.num_nodes == n and g.num_edges == {et: 25 for et in ets}
    assert g.ntypes == ["user", "item"] and g.etypes == ets
    assert gm.num_node_types(g) == 2 and gm.num_edge_types(g) == 3
    for et in ets:
        s, t = gm.edge_index(g, et)
        assert np.array_equal(s.cpu().numpy(), coo[et][0]) and np.array_equal(t.cpu().numpy(), coo[et][1])
        din = gm.degree(g, et, dir="in").cpu().numpy()
        dout = gm.degree(g, et, dir="out").cpu().numpy()
        assert np.array_equal(din, np.bincount(coo[et][1] - 1, minlength=n[et[2]]))
        assert np.array_equal(dout, np.bincount(coo[et][0] - 1, minlength=n[et[0]]))
        assert din.dtype == np.int64
    assert np.array_equal(gm.get_edge_weight(g, ets[0]).cpu().numpy(), w) and gm.get_edge_weight(g, ets[1]) is None
    with pytest.raises(ValueError):
        gm.edge_index(g)                                     # more than one relation: `only` raises
    # the default node counts: the maximum index seen per type
    g2 = gm.GNNHeteroGraph({("a", "to", "b"): ([1, 3], [2, 7]), ("b", "to", "a"): ([9], [1])})
    assert g2.num_nodes == {"a": 3, "b": 9}
    # the index range is asserted at construction
    with pytest.raises(AssertionError):
        gm.GNNHeteroGraph({("a", "to", "b"): ([1, 4], [2, 2])}, num_nodes={"a": 3, "b": 2})
    with pytest.raises(AssertionError):
        gm.GNNHeteroGraph({("a", "to", "b"): ([1, 2], [2, 3])}, num_nodes={"a": 3, "b": 2})
    with pytest.raises(AssertionError):
        gm.GNNHeteroGraph({("a", "to", "b"): ([0, 2], [2, 1])}, num_nodes={"a": 3, "b": 2})
    # features by type
    xu = torch.zeros((9, 2), device="cuda")
    assert gm.GNNHeteroGraph(data, num_nodes=n, ndata={"user": xu})["user"] is xu


def test_subgraph_shares_plans_and_message_passing_scatters_into_the_destination_type(gm):
    import torch
    rng = np.random.default_rng(41)
    et, rev = ("A", "to", "B"), ("B", "to", "A")
    nA, nB, E, D = 7, 12, 30, 5
    s, t = rng.integers(1, nA + 1, E), rng.integers(1, nB + 1, E)
    g = gm.GNNHeteroGraph({et: (s, t), rev: (t, s)}, num_nodes={"A": nA, "B": nB})
    sub = gm.edge_type_subgraph(g, et)
    assert sub.plan() is g.plan(et) and sub.plan_transposed() is g.plan_transposed(et)
    assert gm.edge_type_subgraph(g, [et, rev]).plan(rev) is g.plan(rev)
    assert sub.num_edges == E and sub.index_base == 1 and sub.w is None and sub.num_nodes == {"A": nA, "B": nB}
    assert (sub.plan().n_src, sub.plan().n_dst) == (nA, nB)
    assert np.array_equal(gm.edge_index(sub)[0].cpu().numpy(), s)
    xA, xB = torch.from_numpy(rng.uniform(-1, 1, (nA, D)).astype(np.float32)).cuda(), torch.zeros((nB, D), device="cuda")
    assert gm.check_num_nodes(sub, (xA, xB))
    with pytest.raises(AssertionError):
        gm.check_num_nodes(sub, (xB, xA))                    # swapped sides
    with pytest.raises(AssertionError):
        gm.check_num_edges(sub, torch.zeros((E + 1, 2), device="cuda"))
    assert gm.check_num_edges(sub, torch.zeros((E, 2), device="cuda"))
    y = gm.propagate(gm.copy_xj, sub, "+", xj=xA)
    assert y.shape == (nB, D)
    same_bits(y.cpu().numpy(), R.propagate_ref(s - 1, t - 1, nB, xA.cpu().numpy(), None, "+"), "propagate on a relation")
    m = gm.apply_edges(gm.copy_xj, sub, xj=xA)
    assert m.shape == (E, D)
    z = gm.aggregate_neighbors(sub, "max", m)
    same_bits(z.cpu().numpy(), R.propagate_ref(s - 1, t - 1, nB, xA.cpu().numpy(), None, "max"), "aggregate_neighbors on a relation")
    # a GNNGraph is checked as before
    gg = gm.GNNGraph(s, s, num_nodes=nA)
    assert gm.check_num_nodes(gg, (xA, xA))
    with pytest.raises(AssertionError):
        gm.check_num_nodes(gg, xB)


def test_generators(gm):
    g = gm.rand_bipartite_heterograph((10, 15), 20, seed=3)
    assert g.num_nodes == {"A": 10, "B": 15} and g.num_edges == {("A", "to", "B"): 20, ("B", "to", "A"): 20}
    (s1, t1), (s2, t2) = gm.edge_index(g, ("A", "to", "B")), gm.edge_index(g, ("B", "to", "A"))
    assert bool((s1 == t2).all()) and bool((t1 == s2).all())                     # bidirected: the reverse relation
    g2 = gm.rand_bipartite_heterograph((10, 15), 20, seed=3)
    assert bool((gm.edge_index(g2, ("A", "to", "B"))[0] == s1).all())            # seeded
    h = gm.rand_bipartite_heterograph((2, 2), (4, 0), bidirected=False, seed=1)
    assert h.num_edges == {("A", "to", "B"): 4, ("B", "to", "A"): 0}
    k = gm.rand_heterograph({"u": 10, "m": 20}, {("u", "rate", "m"): 30, ("m", "rate", "u"): 30}, seed=5)
    assert k.num_nodes == {"u": 10, "m": 20} and int(gm.edge_index(k, ("u", "rate", "m"))[1].max()) <= 20


# ------------------------------------------------------------------------------------------------------------------------------------
# the layer
# ------------------------------------------------------------------------------------------------------------------------------------
REF_S, REF_T = np.array([1, 1, 2, 3]), np.array([1, 2, 2, 3])
REF_ETS = [("A", "to", "B"), ("B", "to", "A"), ("C", "to", "A")]


def _layer_params(l, Din):
    from gnnmp import hetero
    wr, wa = hetero._split_weights(l, Din)
    return wr.cpu().numpy(), wa.cpu().numpy(), None if l.bias is None else l.bias.cpu().numpy(), l.sigma, l.aggr


def _conv_ref(model, coo0, num_nodes, x, dtype=np.float64):
    layers = [(et, _layer_params(l, x[et[0]].shape[1])) for et, l in zip(model.etypes, model.layers)]
    return R.hetero_conv_ref(layers, coo0, num_nodes, x, model.aggr, dtype)


@pytest.mark.parametrize("combine", ["+", "max", "min"])
def test_the_reference_three_relation_case(gm, combine):
    """test/layers/heteroconv.jl:39-75: weights of ones, no bias.  `+`: the reference's hand-computed rows; max / min (the reference's
    second operator, `-`, is not in this mirror's set): the same graph against the restatement"""
    import torch
    d, n = 3, 5
    g = gm.GNNHeteroGraph({et: (REF_S, REF_T) for et in REF_ETS}, num_nodes={k: n for k in "ABC"})

    def ones_conv():
        l = gm.GraphConv((d, d), bias=False)
        l.weight1, l.weight2 = torch.ones((d, d), device="cuda"), torch.ones((d, d), device="cuda")
        return l
    model = gm.HeteroGraphConv([(et, ones_conv()) for et in REF_ETS], aggr=combine)
    assert model.etypes == REF_ETS and len(model.layers) == 3 and model.aggr == combine
    rng = np.random.default_rng(43)
    x = {k: rng.random((n, d)).astype(np.float32) for k in "ABC"}
    y = {k: v.cpu().numpy() for k, v in model(g, {k: torch.from_numpy(v).cuda() for k, v in x.items()}).items()}
    assert list(y) == ["B", "A"] and y["A"].shape == (n, d) and y["B"].shape == (n, d)
    ref = _conv_ref(model, {et: (REF_S - 1, REF_T - 1) for et in REF_ETS}, {k: n for k in "ABC"}, x)
    for k in y:
        close64(y[k], ref[k], f"y.{k} ({combine})")
    if combine == "+":
        W = np.ones((d, d))
        col = lambda a, rows: sum(W @ a[r].astype(np.float64) for r in rows)      # noqa: E731
        hand = [("B", 1, col(x["A"], [0, 1]) + W @ x["B"][1]), ("B", 4, W @ x["B"][4]),
                ("A", 0, W @ x["B"][0] + W @ x["C"][0] + 2 * (W @ x["A"][0])),
                ("A", 1, col(x["B"], [0, 1]) + col(x["C"], [0, 1]) + 2 * (W @ x["A"][1])), ("A", 4, 2 * (W @ x["A"][4]))]
        for k, row, want in hand:
            assert np.allclose(y[k][row], want, rtol=1e-5, atol=0), (k, row)


def _random_hetero(gm, rng, nA=31, nB=45, E=140, zero_edges=False):
    ets = [("A", "ab", "B"), ("B", "ba", "A"), ("A", "aa", "A"), ("B", "ba2", "A")]
    n = {"A": nA, "B": nB}
    coo0 = {}
    for k, et in enumerate(ets):
        Ek = 0 if (zero_edges and k in (0, 3)) else E + k
        coo0[et] = (rng.integers(0, n[et[0]], Ek), rng.integers(0, n[et[2]], Ek))
    g = gm.GNNHeteroGraph({et: (s + 1, t + 1) for et, (s, t) in coo0.items()}, num_nodes=n)
    return g, ets, n, coo0


@pytest.mark.parametrize("zero_edges", [False, True])
@pytest.mark.parametrize("kind,aggr", [("graph", "+"), ("graph", "mean"), ("graph", "max"), ("graph", "min"),
                                       ("sage", "mean"), ("sage", "+"), ("sage", "max"), ("sage", "min")])
def test_graphconv_and_sageconv_on_bipartite_relations(gm, monkeypatch, kind, aggr, zero_edges):
    """sigma = relu: the general path (one layer call per relation, outputs folded by identity relations); sigma = None: the fused path
    for + / mean (transform first, ONE hetero launch, no per-relation propagate), the general path for max / min; the knob sends the
    fused case to the composition.  All within 1e-5 of float64."""
    import torch
    from gnnmp import _lib
    rng = np.random.default_rng([5, len(aggr), int(zero_edges)])
    g, ets, n, coo0 = _random_hetero(gm, rng, zero_edges=zero_edges)
    Din, Dout = 12, 8
    x = {k: rng.uniform(-1, 1, (v, Din)).astype(np.float32) for k, v in n.items()}
    xd = {k: torch.from_numpy(v).cuda() for k, v in x.items()}
    Layer = gm.GraphConv if kind == "graph" else gm.SAGEConv
    lib = _lib.load()
    for sigma in ("relu", None):
        layers = [Layer((Din, Dout), sigma, aggr=aggr, seed=50 + k) for k in range(len(ets))]
        for l in layers:
            l.bias = torch.from_numpy(rng.uniform(-1, 1, Dout).astype(np.float32)).cuda()
        model = gm.HeteroGraphConv(dict(zip(ets, layers)), aggr="+")
        ref = _conv_ref(model, coo0, n, x)
        with monkeypatch.context() as mp:
            counts = spy(mp, lib, "gnnmp_hetero_propagate_f32", "gnnmp_propagate_f32")
            y = model(g, xd)
        assert list(y) == ["B", "A"] and y["A"].shape == (n["A"], Dout) and y["B"].shape == (n["B"], Dout)
        fused = sigma is None and aggr in ("+", "mean")
        if fused:
            assert counts == {"gnnmp_hetero_propagate_f32": 1, "gnnmp_propagate_f32": 0}, counts
        else:      # B has one relation (its output itself), A three: one combiner call; a propagate per relation
            assert counts == {"gnnmp_hetero_propagate_f32": 1, "gnnmp_propagate_f32": 4}, counts
        for k in y:
            close64_layer(y[k].cpu().numpy(), ref[k], f"{kind} {aggr} sigma={sigma} y.{k}")
        if fused:
            with _lib.tuned(_lib.Knob.HETERO, -1):
                with monkeypatch.context() as mp:
                    counts = spy(mp, lib, "gnnmp_hetero_propagate_f32", "gnnmp_propagate_f32")
                    y2 = model(g, xd)
            assert counts == {"gnnmp_hetero_propagate_f32": 1, "gnnmp_propagate_f32": 4}, counts
            for k in y:
                close64_layer(y2[k].cpu().numpy(), ref[k], f"{kind} {aggr} composition y.{k}")
                close64_layer(y2[k].cpu().numpy(), y[k].cpu().numpy().astype(np.float64), f"{kind} {aggr} composition against fused y.{k}")


def test_a_wider_output_than_input_takes_the_general_path(gm, monkeypatch):
    import torch
    from gnnmp import _lib
    rng = np.random.default_rng(59)
    g, ets, n, coo0 = _random_hetero(gm, rng)
    x = {k: rng.uniform(-1, 1, (v, 4)).astype(np.float32) for k, v in n.items()}
    model = gm.HeteroGraphConv({et: gm.GraphConv((4, 8), seed=60 + k) for k, et in enumerate(ets)})
    counts = spy(monkeypatch, _lib.load(), "gnnmp_propagate_f32")
    y = model(g, {k: torch.from_numpy(v).cuda() for k, v in x.items()})
    assert counts["gnnmp_propagate_f32"] == 4                # Dout > Din: aggregate first, per relation
    ref = _conv_ref(model, coo0, n, x)
    for k in y:
        close64(y[k].cpu().numpy(), ref[k], f"y.{k}")


def test_layers_that_do_not_take_a_pair_raise_by_name(gm):
    """of the layers the reference's test names, GraphConv and SAGEConv go through expand_srcdst and run on a bipartite relation (shapes
    above, as test/layers/heteroconv.jl:113-119); the others are refused by name, not answered wrongly"""
    import torch
    hg = gm.rand_bipartite_heterograph((2, 3), 6, seed=2)
    x = {"A": torch.rand((2, 4), device="cuda"), "B": torch.rand((3, 4), device="cuda")}
    y = gm.HeteroGraphConv({("A", "to", "B"): gm.SAGEConv((4, 2), torch.tanh, bias=False, aggr="+"),
                            ("B", "to", "A"): gm.SAGEConv((4, 2), torch.tanh, bias=False, aggr="+")})(hg, x)
    assert y["A"].shape == (2, 2) and y["B"].shape == (3, 2)
    y = gm.HeteroGraphConv({("A", "to", "B"): gm.GraphConv((4, 2), "relu"), ("B", "to", "A"): gm.GraphConv((4, 2), "relu")})(hg, x)
    assert y["A"].shape == (2, 2) and y["B"].shape == (3, 2)
    others = {"GCNConv": lambda: gm.GCNConv((4, 2)), "GATConv": lambda: gm.GATConv((4, 2)), "GATv2Conv": lambda: gm.GATv2Conv((4, 2)),
              "GINConv": lambda: gm.GINConv(gm.Dense((4, 2)), 0.4), "CGConv": lambda: gm.CGConv((4, 2)),
              "EdgeConv": lambda: gm.EdgeConv(gm.Dense((8, 2)), aggr="+"), "ResGatedGraphConv": lambda: gm.ResGatedGraphConv((4, 2))}
    for name, make in others.items():
        model = gm.HeteroGraphConv({("A", "to", "B"): make(), ("B", "to", "A"): make()})
        with pytest.raises(NotImplementedError, match=name):
            model(hg, x)
