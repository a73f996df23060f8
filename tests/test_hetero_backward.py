"""The heterograph adjoints on the device: hetero_grad_rows_kernel (csrc/hetero_backward.hip) through gnnmp_hetero_propagate_grad_f32, its
memory contract and its capture into a HIP graph, and the Python adjoints built on it (gnnmp/backward_hetero.py).

Bars: the export is BIT-IDENTICAL to the ordered float32 restatement (tests/hetero_grad_ref.py: slots of a source row in original edge
order, Δ * sd rounded, then w *, the relations' terms added in table order with the first one copied; winners and masked terms are
copies or zeros, so they owe the same bits) and within 1e-5 of the float64 restatement by the comparison of the ABI tests
(abi_cases.compare: norm-wise and element-wise against the reference's scale).  The Python adjoints are held to the 1e-5 bar."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_cases as A  # noqa: E402
import hetero_grad_ref as G  # noqa: E402
import hetero_ref as R  # noqa: E402
import test_hetero as TH  # noqa: E402  (helpers only: spy, close64, same_bits)

pytestmark = pytest.mark.gpu

F32 = np.float32
N_DST = (13, 1, 40, 5)
LINEAR = ("+", "mean", "id", "+w", "meanw")
EXPORT = "gnnmp_hetero_propagate_grad_f32"


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


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------------------------------------------------------------------------
# a synthetic source type: R records of different destination counts (1 included), one relation without edges (R > 2: record 1), source
# rows that are empty in every relation (j % 5 == 3), kinds in turn: "+", "mean" (sd = 1 / count), "id" (identity), "+w", "meanw"
# (weighted), "max" / "min" (winners; x and the forward aggregate y ride along)
# ------------------------------------------------------------------------------------------------------------------------------------
def make_src(rng, n_src, R_, D, kinds=LINEAR, x=None, hub=None):
    rows = np.array([j for j in range(n_src) if j % 5 != 3] or [0])
    rels = []
    for r in range(R_):
        kind = kinds[r % len(kinds)]
        if kind == "id":
            rels.append(dict(kind="id", dy=rng.uniform(-1, 1, (n_src, D)).astype(F32)))
            continue
        n_dst = N_DST[r % 4] + r // 4
        E = 0 if (r == 1 and R_ > 2) else 3 * n_src + r
        s0, t0 = rows[rng.integers(0, len(rows), E)], rng.integers(0, n_dst, E)
        if hub is not None and r == hub[0]:          # hub = (record, source row, out-degree): that row gets exactly that many edges
            extra = hub[2] - int((s0 == hub[1]).sum())
            s0, t0 = np.concatenate([s0, np.full(extra, hub[1])]), np.concatenate([t0, rng.integers(0, n_dst, extra)])
            perm = rng.permutation(len(s0))
            s0, t0 = s0[perm], t0[perm]
        rel = dict(kind=kind, s=s0, t=t0, n_dst=n_dst, dy=rng.uniform(-1, 1, (n_dst, D)).astype(F32))
        if kind.endswith("w"):
            rel["w"] = rng.uniform(0.5, 1.5, len(s0)).astype(F32)
        if kind.startswith("mean"):
            rel["sd"] = F32(1) / np.maximum(np.bincount(t0, minlength=n_dst), 1).astype(F32)
        if kind in ("max", "min"):
            rel["y"] = R.propagate_ref(s0, t0, n_dst, x, None, kind, F32)
        rels.append(rel)
    return rels


def term_ref(rel, n_src, x, dtype):
    if rel["kind"] == "id":
        return rel["dy"].astype(dtype)
    if rel["kind"] == "mask":
        return G.masked_ref(rel["y"], rel["out"], rel["dy"], dtype)
    if rel["kind"] in ("max", "min"):
        return G.winners_ref(rel["s"], rel["t"], n_src, x, rel["y"], rel["dy"], dtype)
    return G.linear_ref(rel["s"], rel["t"], n_src, rel["dy"], rel.get("w"), rel.get("sd"), dtype)


def src_ref(rels, n_src, x, dtype):
    return G.sum_ref([term_ref(rel, n_src, x, dtype) for rel in rels])


class RawCall:
    """one gnnmp_hetero_propagate_grad_f32 call with every array inside abi_cases' poisoned slab.  sources: [(n_src, x | None, records)]"""

    KEYS = ("dy", "w", "sd", "y", "out")

    def __init__(self, sources, D, shift=0, idx=np.int64, base=1):
        from gnnmp.graph import Plan
        self.sources, self.D = sources, D
        arrs = []
        for si, (n_src, x, rels) in enumerate(sources):
            arrs.append(A.Arr(f"dx{si}", "out", shape=(n_src, D)))
            if x is not None:
                arrs.append(A.Arr(f"x{si}", "in", x))
            for ri, rel in enumerate(rels):
                arrs += [A.Arr(f"{k}{si}_{ri}", "in", rel[k]) for k in self.KEYS if rel.get(k) is not None and rel[k].size]
        self.slab = A.Slab(arrs, "cuda", {a.name: shift for a in arrs})
        # the TRANSPOSED plan of a relation: built from (t, s) — rows = source nodes, col = destination
        self.plans = {(si, ri): Plan(_dev((rel["t"] + base).astype(idx)), _dev((rel["s"] + base).astype(idx)), rel["n_dst"], n_src, base, False)
                      for si, (n_src, _, rels) in enumerate(sources) for ri, rel in enumerate(rels) if "s" in rel}
        self.keep = []

    def ptr(self, name):
        return self.slab.ptr(name) if name in self.slab.arrs else None

    def tables(self):
        from gnnmp import _lib
        srcs = (_lib.HeteroSrc * len(self.sources))()
        for si, (s, (n_src, x, rels)) in enumerate(zip(srcs, self.sources)):
            tab = (_lib.HeteroRelGrad * len(rels))()
            for ri, (q, rel) in enumerate(zip(tab, rels)):
                q.plan_t = self.plans[(si, ri)].handle if (si, ri) in self.plans else None
                q.dy, q.w, q.sd, q.y, q.out = (self.ptr(f"{k}{si}_{ri}") for k in self.KEYS)
            self.keep.append(tab)
            s.dx, s.x, s.n_src, s.n_rel, s.rels = self.ptr(f"dx{si}"), self.ptr(f"x{si}"), n_src, len(rels), tab
        return srcs

    def run(self, stream=None):
        from gnnmp import _lib
        return _lib.load().gnnmp_hetero_propagate_grad_f32(self.tables(), len(self.sources), self.D, stream)

    def reference(self, data=None, dtype=F32):
        """{dx: expected} for the arrays as they are in the slab (data: {array name: new values})"""
        data = data or {}
        ref = {}
        for si, (n_src, x, rels) in enumerate(self.sources):
            now = [dict(rel, **{k: data[f"{k}{si}_{ri}"] for k in self.KEYS if f"{k}{si}_{ri}" in data}) for ri, rel in enumerate(rels)]
            ref[f"dx{si}"] = src_ref(now, n_src, data.get(f"x{si}", x), dtype)
        return ref

    def check(self, what):
        """bit-equal to the float32 restatement, every output element written, no stray store, inputs untouched; 1e-5 of float64"""
        import torch
        torch.cuda.synchronize()
        problems = self.slab.check({k: A.E(v, "exact") for k, v in self.reference().items()})
        assert not problems, what + ":\n" + "\n".join(problems)
        out = self.slab.outputs()
        for k, v in self.reference(dtype=np.float64).items():
            TH.close64(out[k].view(F32).reshape(v.shape), v, f"{what} {k} against float64")


# ------------------------------------------------------------------------------------------------------------------------------------
# the kernel
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_src", [1, 31, 33, 300])
@pytest.mark.parametrize("R_", [1, 2, "cap"])
@pytest.mark.parametrize("D", [1, 3, 4, 100, 260])
def test_linear_and_identity_modes_match_the_ordered_restatement(gm, cap, D, R_, n_src):
    from gnnmp import _lib
    Rn = cap if R_ == "cap" else R_
    rng = np.random.default_rng([D, Rn, n_src])
    c = RawCall([(n_src, None, make_src(rng, n_src, Rn, D))], D)
    assert c.run() == _lib.OK, _lib.load().gnnmp_last_error()
    c.check(f"D={D} R={Rn} n_src={n_src}")


@pytest.mark.parametrize("D", [3, 100])
@pytest.mark.parametrize("n_src", [33, 300])
def test_winners_and_masked_identity_modes_with_exact_ties(gm, D, n_src):
    """duplicated source rows compete for the same maxima: every tie receives Δ.  The masked records pull back foldl(max) over three terms
    of which two are the same matrix: both receive Δ where they win."""
    from gnnmp import _lib
    rng = np.random.default_rng([7, D, n_src])
    x = rng.uniform(-1, 1, (n_src, D)).astype(F32)
    x[1::2] = x[0:n_src - 1:2][: len(x[1::2])]              # row 2k + 1 repeats row 2k
    rels = make_src(rng, n_src, 5, D, kinds=("max", "+w", "min", "id", "max"), x=x)
    ties = G.winners_ref(rels[0]["s"], rels[0]["t"], n_src, x, rels[0]["y"], np.ones_like(rels[0]["dy"]), F32)
    assert (ties[0::2][: len(ties[1::2])] * ties[1::2] > 0).any(), "no destination sees a row and its copy: the tie is not exercised"
    terms = [rng.uniform(-1, 1, (n_src, D)).astype(F32) for _ in range(2)]
    terms.append(terms[0].copy())
    out = R.fold_ref(terms, "max")
    dy = rng.uniform(-1, 1, (n_src, D)).astype(F32)
    masked = [(n_src, None, [dict(kind="mask", y=t, out=out, dy=dy)]) for t in terms]
    both = dict(kind="mask", y=terms[1], out=R.fold_ref(terms, "min"), dy=dy)
    c = RawCall([(n_src, x, rels + [both])] + masked, D)
    assert c.run() == _lib.OK, _lib.load().gnnmp_last_error()
    c.check(f"winners / masked D={D} n_src={n_src}")
    got = c.slab.outputs()
    d1, d3 = (got[k].view(F32).reshape(n_src, D) for k in ("dx1", "dx3"))
    assert np.array_equal(d1, d3) and np.array_equal(d1, np.where(terms[0] == out, dy, 0)) and (d1 != 0).any()


# ------------------------------------------------------------------------------------------------------------------------------------
# the Python layer on real heterographs: relation r of source type `name` goes to a destination type of its own
# ------------------------------------------------------------------------------------------------------------------------------------
OP = {"+": "+", "+w": "+", "mean": "mean", "meanw": "mean", "max": "max", "min": "min"}


def build_hetero(gm, sources, idx=np.int64, base=1):
    """sources: {name: (n_src, x, records)} -> (graph, the arguments of hetero_propagate_grad)"""
    data, num_nodes, dy, aggr, ew, saved, xs = {}, {}, {}, {}, {}, {}, {}
    for name, (n_src, x, rels) in sources.items():
        num_nodes[name] = n_src
        xs[name] = _dev(x)
        for r, rel in enumerate(rels):
            et = (name, "r", f"{name}_d{r}")
            data[et] = (_dev((rel["s"] + base).astype(idx)), _dev((rel["t"] + base).astype(idx)))
            num_nodes[et[2]] = rel["n_dst"]
            dy[et[2]], aggr[et] = _dev(rel["dy"]), OP[rel["kind"]]
            if "w" in rel:
                ew[et] = _dev(rel["w"])
            if "y" in rel:
                saved[et] = _dev(rel["y"])
    g = gm.GNNHeteroGraph(data, num_nodes=num_nodes, index_base=base)
    return g, dict(dy=dy, x=xs, aggr=aggr, edge_weight=ew, saved=saved)


def value64(rels, n_src, x):
    """the float64 value: 1 / count exact, not the float32 factor the export is handed"""
    exact = [dict(rel, sd=1.0 / np.maximum(np.bincount(rel["t"], minlength=rel["n_dst"]), 1)) if "sd" in rel else rel for rel in rels]
    return src_ref(exact, n_src, x, np.float64)


WALKS = ("+", "mean", "max", "+w", "meanw", "min")
COUNTED = (EXPORT, "gnnmp_propagate_f32", "gnnmp_propagate_maxmin_grad_f32", "gnnmp_hetero_propagate_f32")


def two_sources(rng, D):
    xa, xb = (rng.uniform(-1, 1, (n, D)).astype(F32) for n in (33, 300))
    return {"a": (33, xa, make_src(rng, 33, 3, D, WALKS, xa)), "b": (300, xb, make_src(rng, 300, 6, D, WALKS, xb))}


def test_two_source_types_in_one_launch_and_a_type_that_is_no_source(gm, monkeypatch):
    """two source types of different sizes — through the export also with an identity term on one of them — and ONE call; the destination
    types are no relation's source and come back as zeros"""
    from gnnmp import _lib
    D = 100
    rng = np.random.default_rng(11)
    sources = two_sources(rng, D)
    g, args = build_hetero(gm, sources)
    counts = TH.spy(monkeypatch, _lib.load(), *COUNTED)
    dx = gm.hetero_propagate_grad(g, **args)
    assert counts == {EXPORT: 1, "gnnmp_propagate_f32": 0, "gnnmp_propagate_maxmin_grad_f32": 0, "gnnmp_hetero_propagate_f32": 0}
    assert list(dx) == g.ntypes
    for name, (n, x, rels) in sources.items():
        TH.close64(dx[name].cpu().numpy(), value64(rels, n, x), f"Δx[{name}]")
    for nt in g.ntypes:
        if nt not in sources:
            assert dx[nt].shape == (g.num_nodes[nt], D) and not bool(dx[nt].any()), nt
    # the same two types through the export, type a with an identity term in front: bit-equal to the ordered restatement
    ident = dict(kind="id", dy=rng.uniform(-1, 1, (33, D)).astype(F32))
    c = RawCall([(33, sources["a"][1], [ident] + sources["a"][2]), (300, sources["b"][1], sources["b"][2])], D)
    assert c.run() == _lib.OK, _lib.load().gnnmp_last_error()
    c.check("two source types")


@pytest.mark.parametrize("idx,base", [(np.int64, 1), (np.int32, 1), (np.int64, 0), (np.int32, 0)])
def test_index_widths_and_bases(gm, idx, base):
    from gnnmp import _lib
    rng = np.random.default_rng(13)
    x = rng.uniform(-1, 1, (33, 4)).astype(F32)
    rels = make_src(rng, 33, 6, 4, WALKS, x)
    g, args = build_hetero(gm, {"a": (33, x, rels)}, idx, base)
    assert g.idx_bytes == np.dtype(idx).itemsize and g.index_base == base
    TH.close64(gm.hetero_propagate_grad(g, **args)["a"].cpu().numpy(), value64(rels, 33, x), f"{idx.__name__} base {base}")
    c = RawCall([(33, x, rels)], 4, idx=idx, base=base)
    assert c.run() == _lib.OK, _lib.load().gnnmp_last_error()
    c.check(f"{idx.__name__} base {base}")


def test_a_source_row_of_five_times_the_split_threshold(gm, monkeypatch):
    """the export walks a split row whole, in edge order: the bits of the sequential loop; hetero_propagate_grad sends the graph to the
    composition (a transposed propagate, a max adjoint, and the forward kernel's identity relations as the sum)"""
    from gnnmp import _lib
    D, n_src = 100, 33
    rng = np.random.default_rng(17)
    thr = _lib.LONG_ROW // 8                                 # the threshold of a small plan — read back below
    x = rng.uniform(-1, 1, (n_src, D)).astype(F32)
    rels = make_src(rng, n_src, 2, D, ("max", "+w"), x, hub=(1, 7, 5 * thr))
    g, args = build_hetero(gm, {"a": (n_src, x, rels)})
    pt = g.plan(("a", "r", "a_d1"), transposed=True)
    assert pt.long_thresh == thr and pt.n_long == 1 and int((rels[1]["s"] == 7).sum()) == 5 * thr
    counts = TH.spy(monkeypatch, _lib.load(), *COUNTED)
    dx = gm.hetero_propagate_grad(g, **args)["a"].cpu().numpy()
    assert counts == {EXPORT: 0, "gnnmp_propagate_f32": 1, "gnnmp_propagate_maxmin_grad_f32": 1, "gnnmp_hetero_propagate_f32": 1}
    TH.close64(dx, value64(rels, n_src, x), "the composition on a split row")
    c = RawCall([(n_src, x, rels)], D)
    assert c.plans[(0, 1)].n_long == 1
    assert c.run() == _lib.OK, _lib.load().gnnmp_last_error()
    c.check("the export on a split row")
    short = np.arange(n_src) != 7
    TH.same_bits(dx[short], c.reference()["dx0"][short], "the composition on the rows that are not split")


def test_the_knob_and_the_cap_send_the_call_to_the_composition(gm, cap, monkeypatch):
    from gnnmp import _lib
    D = 4
    rng = np.random.default_rng(19)
    x = rng.uniform(-1, 1, (31, D)).astype(F32)
    rels = make_src(rng, 31, cap + 1, D, WALKS, x)
    g, args = build_hetero(gm, {"a": (31, x, rels)})
    n_win = sum(rel["kind"] in ("max", "min") for rel in rels)
    with monkeypatch.context() as mp:
        counts = TH.spy(mp, _lib.load(), *COUNTED)
        over = gm.hetero_propagate_grad(g, **args)["a"].cpu().numpy()
    assert counts == {EXPORT: 0, "gnnmp_propagate_f32": cap + 1 - n_win, "gnnmp_propagate_maxmin_grad_f32": n_win, "gnnmp_hetero_propagate_f32": 2}
    TH.close64(over, value64(rels, 31, x), "cap + 1 relations")
    # within the cap: one launch, and the composition under the knob gives the same bits (no split rows)
    g, args = build_hetero(gm, {"a": (31, x, rels[:6])})
    one = gm.hetero_propagate_grad(g, **args)["a"].cpu().numpy()
    counts = TH.spy(monkeypatch, _lib.load(), *COUNTED)
    with _lib.tuned(_lib.Knob.HETERO, -1):
        two = gm.hetero_propagate_grad(g, **args)["a"].cpu().numpy()
    assert counts == {EXPORT: 0, "gnnmp_propagate_f32": 4, "gnnmp_propagate_maxmin_grad_f32": 2, "gnnmp_hetero_propagate_f32": 1}
    TH.same_bits(two, one, "the composition against the one-launch kernel")
    TH.close64(one, value64(rels[:6], 31, x), "six relations")


# ------------------------------------------------------------------------------------------------------------------------------------
# the memory contract and capture
# ------------------------------------------------------------------------------------------------------------------------------------
def slab_call(D, shift=0, seed=23):
    """two source types (33 and 300 rows), every mode: identity, weighted and unweighted + / mean, max and min, a masked identity"""
    rng = np.random.default_rng(seed)
    xa, xb = (rng.uniform(-1, 1, (n, D)).astype(F32) for n in (33, 300))
    a = make_src(rng, 33, 4, D, ("id", "+w", "max", "mean"), xa)
    b = make_src(rng, 300, 5, D, ("meanw", "min", "+", "id", "+w"), xb)
    term = rng.uniform(-1, 1, (300, D)).astype(F32)
    out = np.maximum(term, rng.uniform(-1, 1, (300, D)).astype(F32))
    b.append(dict(kind="mask", y=term, out=out, dy=rng.uniform(-1, 1, (300, D)).astype(F32)))
    return RawCall([(33, xa, a), (300, xb, b)], D, shift=shift)


@pytest.mark.parametrize("shift", [0, 4, 8])
@pytest.mark.parametrize("D", [100, 3, 260])
def test_writes_all_of_dx_and_nothing_else(gm, D, shift):
    """every element of both dx written, no stray store, the inputs untouched — at natural alignment and with every pointer shifted to
    4-byte (8-byte) alignment, where the 16-byte lanes must give way to narrower ones"""
    from gnnmp import _lib
    c = slab_call(D, shift)
    assert c.run() == _lib.OK, _lib.load().gnnmp_last_error()
    c.check(f"D={D} shift={shift}")


def test_a_refused_call_leaves_the_slab_untouched(gm, cap):
    import torch
    from gnnmp import _lib
    lib = _lib.load()
    c = slab_call(100)
    t = c.tables()
    assert lib.gnnmp_hetero_propagate_grad_f32(t, 2, 0, None) == _lib.EINVAL
    t[1].rels[1].w = c.slab.ptr("w1_0")                      # a max / min record with edge weights
    assert lib.gnnmp_hetero_propagate_grad_f32(t, 2, 100, None) == _lib.EINVAL and b"together with w or sd" in lib.gnnmp_last_error()
    t = c.tables()
    t[1].rels[5].y = None                                    # out without y
    assert lib.gnnmp_hetero_propagate_grad_f32(t, 2, 100, None) == _lib.EINVAL and b"out without y" in lib.gnnmp_last_error()
    t = c.tables()
    t[0].n_src = 34                                          # the plans have 33 rows
    assert lib.gnnmp_hetero_propagate_grad_f32(t, 2, 100, None) == _lib.EINVAL and b"rows" in lib.gnnmp_last_error()
    t = c.tables()
    t[1].n_rel = cap                                         # 4 + cap records announced
    assert lib.gnnmp_hetero_propagate_grad_f32(t, 2, 100, None) == _lib.EUNSUPPORTED
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
    c = slab_call(D)
    exact = lambda ref: {k: A.E(v, "exact") for k, v in ref.items()}      # noqa: E731
    ref0 = exact(c.reference())
    srcs = c.tables()
    side = torch.cuda.Stream()
    sp = ctypes.c_void_p(side.cuda_stream)
    torch.cuda.synchronize()

    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        graph.capture_begin(capture_error_mode="thread_local")
        try:
            rc = lib.gnnmp_hetero_propagate_grad_f32(srcs, 2, D, sp)
        finally:
            graph.capture_end()
            torch.cuda.synchronize()
    assert rc == _lib.OK, lib.gnnmp_last_error()
    problems = c.slab.check({}, untouched=True)
    assert not problems, "work ran while the call was being recorded: " + "\n".join(problems)

    graph.replay()
    torch.cuda.synchronize()
    problems = c.slab.check(ref0)
    assert not problems, "replay 1: " + "\n".join(problems)
    first = c.slab.outputs()

    c.slab.reload()
    assert lib.gnnmp_hetero_propagate_grad_f32(srcs, 2, D, sp) == _lib.OK                            # the eager call, same stream
    torch.cuda.synchronize()
    eager = c.slab.outputs()
    assert all(np.array_equal(first[k], eager[k]) for k in eager), "replay 1 differs from the eager call"

    # new values in the same buffers; the graph-dependent arrays (a max / min relation's y must stay the aggregate of ITS x) keep theirs
    rng = np.random.default_rng(31)
    new = {a.name: (rng.uniform(0.5, 1.5, a.shape) if a.name.startswith(("w", "sd")) else rng.uniform(-1, 1, a.shape)).astype(F32)
           for a in c.slab.arrs.values() if a.role == "in" and a.name.startswith(("dy", "w", "sd"))}
    ref1 = exact(c.reference(new))
    c.slab.reload(new)
    graph.replay()
    torch.cuda.synchronize()
    problems = c.slab.check(ref1)
    assert not problems, "replay 2, new values in the same buffers: " + "\n".join(problems)
    second = c.slab.outputs()
    assert any(not np.array_equal(first[k], second[k]) for k in second)

    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    last = c.slab.outputs()
    assert all(np.array_equal(last[k], second[k]) for k in second), "two replays back to back differ from replay 2"
    del graph


# ------------------------------------------------------------------------------------------------------------------------------------
# hetero_propagate_ad: the reference's three-relation item (test/layers/heteroconv.jl:39-75: A -> B, B -> A, C -> A on 5 + 5 + 5 nodes)
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combine", ["+", "max", "min"])
def test_hetero_propagate_ad_gradients_of_x_root_and_w(gm, combine):
    import torch
    d, n = 3, 5
    ets = TH.REF_ETS
    s0, t0 = TH.REF_S - 1, TH.REF_T - 1
    g = gm.GNNHeteroGraph({et: (TH.REF_S, TH.REF_T) for et in ets}, num_nodes={k: n for k in "ABC"})
    rng = np.random.default_rng([37, len(combine)])
    aggr = dict(zip(ets, ("+", "mean", "max")))
    x = {k: rng.uniform(-1, 1, (n, d)).astype(F32) for k in "ABC"}
    root = {k: rng.uniform(-1, 1, (n, d)).astype(F32) for k in "AB"}
    w = {ets[0]: rng.uniform(0.5, 1.5, 4).astype(F32), ets[1]: rng.uniform(0.5, 1.5, 4).astype(F32)}
    dout = {k: rng.uniform(-1, 1, (n, d)).astype(F32) for k in "BA"}
    leaf = lambda v: _dev(v).requires_grad_(True)           # noqa: E731
    xd, rd, wd = ({k: leaf(v) for k, v in m.items()} for m in (x, root, w))
    y = gm.hetero_propagate_ad(g, xd, aggr=aggr, combine=combine, edge_weight=wd, root=rd)
    assert list(y) == ["B", "A"]
    plain = gm.hetero_propagate(g, {k: _dev(v) for k, v in x.items()}, aggr=aggr, combine=combine,
                                edge_weight={k: _dev(v) for k, v in w.items()}, root={k: _dev(v) for k, v in root.items()})
    for k in y:
        assert torch.equal(y[k].detach(), plain[k]) or np.array_equal(y[k].detach().cpu().numpy(), plain[k].cpu().numpy(), equal_nan=True), k
    inputs = list(xd.values()) + list(rd.values()) + list(wd.values())
    grads = torch.autograd.grad([y[k] for k in y], inputs, grad_outputs=[_dev(dout[k]) for k in y])
    gx = dict(zip(xd, grads[:3]))
    groot = dict(zip(rd, grads[3:5]))
    gw = dict(zip(wd, grads[5:]))
    dx = {k: np.zeros((n, d)) for k in "ABC"}
    for dst in "BA":
        mine = [et for et in ets if et[2] == dst]
        droot, res = G.hetero_grad_ref([(s0, t0, x[et[0]], w.get(et), aggr[et]) for et in mine], n, dout[dst], combine, root=root[dst])
        TH.close64(groot[dst].cpu().numpy(), droot, f"Δroot[{dst}] ({combine})")
        for et, (dxr, dwr) in zip(mine, res):
            dx[et[0]] += dxr
            if et in w:
                TH.close64(gw[et].cpu().numpy(), dwr, f"Δw[{et}] ({combine})")
    for k in "ABC":
        TH.close64(gx[k].cpu().numpy(), dx[k], f"Δx[{k}] ({combine})")


# ------------------------------------------------------------------------------------------------------------------------------------
# hetero_conv_ad: a 3-type graph of a few dozen nodes
# ------------------------------------------------------------------------------------------------------------------------------------
CONV_ETS = [("A", "ab", "B"), ("C", "cb", "B"), ("B", "ba", "A"), ("A", "ab2", "B")]
CONV_N = {"A": 17, "B": 12, "C": 9}


def conv_graph(gm, rng):
    """every destination has one to three DISTINCT sources in every relation: no ∓Inf aggregate under max, no edge twice"""
    coo0 = {}
    for et in CONV_ETS:
        pairs = [(j, i) for i in range(CONV_N[et[2]]) for j in rng.choice(CONV_N[et[0]], rng.integers(1, 4), replace=False)]
        pairs = [pairs[k] for k in rng.permutation(len(pairs))]
        coo0[et] = (np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs]))
    g = gm.GNNHeteroGraph({et: (s + 1, t + 1) for et, (s, t) in coo0.items()}, num_nodes=CONV_N)
    return g, coo0


def conv_model(gm, rng, kind, sigma, aggr, outer, Din=12, Dout=8):
    Layer = gm.GraphConv if kind == "graph" else gm.SAGEConv
    layers = [Layer((Din, Dout), sigma, aggr=aggr, seed=70 + k) for k in range(len(CONV_ETS))]
    for l in layers:
        l.bias = _dev(rng.uniform(-1, 1, Dout).astype(F32))
    return gm.HeteroGraphConv(dict(zip(CONV_ETS, layers)), aggr=outer)


def leaves(model):
    """every parameter tensor of the model as a leaf that requires a gradient: [(member, attribute)]"""
    names = []
    for l in model.layers:
        for attr in ("weight1", "weight2", "weight", "bias"):
            if getattr(l, attr, None) is not None:
                setattr(l, attr, getattr(l, attr).detach().clone().requires_grad_(True))
                names.append((l, attr))
    return names


@pytest.mark.parametrize("outer", ["+", "max"])
@pytest.mark.parametrize("aggr", ["+", "mean", "max"])
@pytest.mark.parametrize("sigma", [None, "relu"])
@pytest.mark.parametrize("kind", ["graph", "sage"])
def test_hetero_conv_ad_gradients_of_x_and_every_parameter(gm, kind, sigma, aggr, outer):
    import torch
    Din = 12
    rng = np.random.default_rng([41, len(aggr), len(outer), sigma is None, kind == "sage"])
    g, coo0 = conv_graph(gm, rng)
    model = conv_model(gm, rng, kind, sigma, aggr, outer)
    x = {k: rng.uniform(-1, 1, (n, Din)).astype(F32) for k, n in CONV_N.items()}
    params = [(et, TH._layer_params(l, Din)) for et, l in zip(model.etypes, model.layers)]
    names = leaves(model)
    xd = {k: _dev(v).requires_grad_(True) for k, v in x.items()}
    y = gm.hetero_conv_ad(model, g, xd)
    assert list(y) == ["B", "A"]
    ref = R.hetero_conv_ref(params, coo0, CONV_N, x, outer, np.float64)
    for k in y:
        TH.close64(y[k].detach().cpu().numpy(), ref[k], f"y.{k}")
    dout = {k: rng.uniform(-1, 1, tuple(v.shape)).astype(F32) for k, v in y.items()}
    grads = torch.autograd.grad([y[k] for k in y], list(xd.values()) + [getattr(l, a) for l, a in names],
                                grad_outputs=[_dev(dout[k]) for k in y])
    dx, dparams = G.hetero_conv_grad_ref(params, coo0, CONV_N, x, dout, outer)
    what = f"{kind} sigma={sigma} aggr={aggr} outer={outer}"
    for k, got in zip(xd, grads[:3]):
        TH.close64(got.cpu().numpy(), dx[k], f"Δx[{k}] {what}")
    got = dict(zip([(id(l), a) for l, a in names], grads[3:]))
    for l, (dWr, dWa, db) in zip(model.layers, dparams):
        if kind == "graph":
            TH.close64(got[(id(l), "weight1")].cpu().numpy(), dWr, f"ΔW_root {what}")
            TH.close64(got[(id(l), "weight2")].cpu().numpy(), dWa, f"ΔW_agg {what}")
        else:
            TH.close64(got[(id(l), "weight")].cpu().numpy(), np.concatenate([dWr, dWa], axis=1), f"ΔW {what}")
        TH.close64(got[(id(l), "bias")].cpu().numpy(), db, f"Δb {what}")


def test_hetero_conv_ad_backward_is_one_grad_launch_for_all_source_types(gm, monkeypatch):
    import torch
    from gnnmp import _lib
    rng = np.random.default_rng(43)
    g, _ = conv_graph(gm, rng)
    model = conv_model(gm, rng, "graph", "relu", "mean", "+")
    names = leaves(model)
    xd = {k: _dev(rng.uniform(-1, 1, (n, 12)).astype(F32)).requires_grad_(True) for k, n in CONV_N.items()}
    y = gm.hetero_conv_ad(model, g, xd)
    loss = sum(v.sum() for v in y.values())
    counts = TH.spy(monkeypatch, _lib.load(), *COUNTED)
    grads = torch.autograd.grad(loss, list(xd.values()) + [getattr(l, a) for l, a in names])
    assert counts == {EXPORT: 1, "gnnmp_propagate_f32": 0, "gnnmp_propagate_maxmin_grad_f32": 0, "gnnmp_hetero_propagate_f32": 0}
    assert all(bool(torch.isfinite(v).all()) for v in grads)
