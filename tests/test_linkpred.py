"""Link prediction (GraphNeuralNetworks/examples/link_prediction_pubmed.jl): negative_sample / rand_edge_split
(GNNGraphs/src/transform.jl:890-968), DotDecoder and the adjoint of the per-edge dot product.

The float64 numpy restatements below follow the reference line by line (randsubseq -> setdiff! -> union! -> truncate; randperm ->
split -> mirror); they are pinned to the reference's own test items (GNNGraphs/test/transform.jl:324-360) without a GPU, and the
device versions are checked against them: exactly where the result is determined, distributionally where it is random."""
import types

import numpy as np
import pytest


# ---------------------------------------------------------------------------------------------------------
# numpy restatements (1-based s, t like the reference)
# ---------------------------------------------------------------------------------------------------------
def ref_sample_prob(n, E, num_neg):
    maxid = float(n) * n
    if maxid == 0:
        return 0.0
    pneg = 1.0 - (E + n) / (2.0 * maxid)
    return 1.0 if pneg == 0 else min(1.0, num_neg / (pneg * maxid) * 1.1)


def ref_negative_sample(s, t, n, num_neg_edges, bidirected, rng, max_trials=3):
    """transform.jl:890-929"""
    s, t = np.asarray(s, np.int64), np.asarray(t, np.int64)
    if num_neg_edges < 0:
        raise ValueError("num_neg_edges < 0")
    pos = np.concatenate([(s - 1) * n + t, np.arange(n, dtype=np.int64) * n + np.arange(1, n + 1)])   # + add_self_loops
    num = num_neg_edges // 2 if bidirected else num_neg_edges
    p = ref_sample_prob(n, len(s), num)
    if p < 0:
        raise ValueError("sample probability < 0")
    idx_neg = np.zeros(0, np.int64)
    for _ in range(max_trials):
        rnd = np.nonzero(rng.random(n * n) < p)[0].astype(np.int64) + 1      # randsubseq(1:maxid, p), ascending
        rnd = rnd[~np.isin(rnd, pos)]                                       # setdiff!
        idx_neg = np.concatenate([idx_neg, rnd[~np.isin(rnd, idx_neg)]])     # union!
        if len(idx_neg) >= num:
            idx_neg = idx_neg[:num]
            break
    sn, tn = (idx_neg - 1) // n + 1, (idx_neg - 1) % n + 1
    if bidirected:
        sn, tn = np.concatenate([sn, tn]), np.concatenate([tn, sn])
    return sn, tn


def ref_rand_edge_split(s, t, frac, bidirected, rng):
    """transform.jl:945-968"""
    if not 0 <= frac <= 1:
        raise ValueError("frac outside [0, 1]")
    s, t = np.asarray(s, np.int64), np.asarray(t, np.int64)
    ne = len(s) // 2 if bidirected else len(s)
    eids = rng.permutation(ne)
    size1 = int(round(ne * frac))
    if bidirected:
        mask = s < t
        s, t = s[mask], t[mask]
        if len(s) < ne:
            raise IndexError("fewer than num_edges / 2 edges with s < t")
    s1, t1 = s[eids[:size1]], t[eids[:size1]]
    s2, t2 = s[eids[size1:]], t[eids[size1:]]
    if bidirected:
        s1, t1 = np.concatenate([s1, t1]), np.concatenate([t1, s1])
        s2, t2 = np.concatenate([s2, t2]), np.concatenate([t2, s2])
    return (s1, t1), (s2, t2)


def rand_graph(n, m, bidirected, rng, self_loops=False):
    """GNNGraphs.rand_graph(n, m; bidirected): m distinct edges (m / 2 distinct pairs and their reverses when bidirected)"""
    if bidirected:
        assert m % 2 == 0
        codes = rng.choice(n * (n - 1) // 2, m // 2, replace=False)
        iu = np.triu_indices(n, 1)
        a, b = iu[0][codes] + 1, iu[1][codes] + 1
        return np.concatenate([a, b]), np.concatenate([b, a])
    codes = rng.choice(n * n, m, replace=False) if self_loops else None
    if codes is None:
        offdiag = np.array([i * n + j for i in range(n) for j in range(n) if i != j])
        codes = rng.choice(offdiag, m, replace=False)
    return codes // n + 1, codes % n + 1


def is_bidirected_np(s, t):
    return sorted(zip(s.tolist(), t.tolist())) == sorted(zip(t.tolist(), s.tolist()))


def edge_set(s, t):
    return set(zip(np.asarray(s).tolist(), np.asarray(t).tolist()))


# ---------------------------------------------------------------------------------------------------------
# without a GPU: the restatements against the reference's test items, and argument validation
# ---------------------------------------------------------------------------------------------------------
def test_reference_items_negative_sample_restatement():
    rng = np.random.default_rng(0)
    n, m = 10, 30
    s, t = rand_graph(n, m, True, rng)
    sn, tn = ref_negative_sample(s, t, n, 20, is_bidirected_np(s, t), rng)
    assert len(sn) == 20
    assert is_bidirected_np(sn, tn)
    assert not (edge_set(s, t) & edge_set(sn, tn))
    assert np.all(sn != tn)


def test_reference_items_rand_edge_split_restatement():
    rng = np.random.default_rng(1)
    n, m = 100, 300
    for bidir in (True, False):
        s, t = rand_graph(n, m, bidir, rng)
        (s1, t1), (s2, t2) = ref_rand_edge_split(s, t, 0.9, is_bidirected_np(s, t), rng)
        assert is_bidirected_np(s1, t1) == bidir and is_bidirected_np(s2, t2) == bidir
        assert not (edge_set(s1, t1) & edge_set(s2, t2))
        assert len(s1) + len(s2) == m
        assert len(s2) < 50


def test_sample_prob_formula_edge_cases():
    assert ref_sample_prob(0, 0, 5) == 0.0
    assert ref_sample_prob(1, 1, 5) == 1.0               # pneg = 0
    assert ref_sample_prob(1, 5, 5) < 0                  # more positives than 2 n^2
    from gnnmp.linkpred import negative_sample_prob
    for n, E, k in [(0, 0, 3), (1, 1, 4), (1, 5, 5), (10, 30, 10), (19717, 88648 + 0, 44324), (2449029, 123718280, 61859140)]:
        assert negative_sample_prob(n, E, k) == ref_sample_prob(n, E, k)


def _fake_graph(n, E, num_graphs=1):
    """stands in for a GNNGraph: validation must raise before any attribute that needs the device is read"""
    return types.SimpleNamespace(num_nodes=n, num_edges=E, num_graphs=num_graphs)


def test_negative_sample_validates_before_launch():
    import gnnmp
    with pytest.raises(AssertionError):
        gnnmp.negative_sample(_fake_graph(10, 20, num_graphs=2), bidirected=False)
    with pytest.raises(ValueError):
        gnnmp.negative_sample(_fake_graph(10, 20), num_neg_edges=-1, bidirected=False)
    with pytest.raises(ValueError):
        gnnmp.negative_sample(_fake_graph(1, 5), num_neg_edges=5, bidirected=False)   # sample_prob < 0


def test_rand_edge_split_validates_before_launch():
    import gnnmp
    for frac in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            gnnmp.rand_edge_split(_fake_graph(10, 20), frac, bidirected=False)


def test_entry_points_validate_without_gpu():
    """the C entry points refuse bad arguments before any HIP call"""
    import ctypes
    from gnnmp import _lib
    lib = _lib.load()
    tot = ctypes.c_int64(0)
    assert lib.gnnmp_negative_sample(None, None, 4, 1, 0, 10, -1, 0, 3, 0, None, None, 0, ctypes.byref(tot), None) == _lib.EINVAL
    assert lib.gnnmp_negative_sample(None, None, 4, 1, 5, 1, 5, 0, 3, 0, None, None, 5, ctypes.byref(tot), None) == _lib.EINVAL
    assert b"probability" in lib.gnnmp_last_error()
    assert lib.gnnmp_negative_sample(None, None, 4, 1, 0, 10, 8, 0, 3, 0, None, None, 7, ctypes.byref(tot), None) == _lib.EINVAL
    assert lib.gnnmp_negative_sample(None, None, 4, 1, 0, 10, 0, 0, 3, 0, None, None, 0, ctypes.byref(tot), None) == _lib.OK
    assert tot.value == 0
    assert lib.gnnmp_rand_edge_split(None, None, 4, 1, 10, 0, 11, 0, None, None, None, None, None) == _lib.EINVAL
    assert lib.gnnmp_rand_edge_split(None, None, 3, 1, 10, 0, 1, 0, None, None, None, None, None) == _lib.EINVAL
    assert lib.gnnmp_edge_dot_grad_f32(None, None, None, None, None, None, None, 4, None) == _lib.EINVAL


# ---------------------------------------------------------------------------------------------------------
# on the GPU
# ---------------------------------------------------------------------------------------------------------
def _graph(s, t, n, dtype="int64", base=1):
    import torch
    import gnnmp
    dt = torch.int64 if dtype == "int64" else torch.int32
    s = torch.as_tensor(np.asarray(s) - 1 + base, dtype=dt).cuda()
    t = torch.as_tensor(np.asarray(t) - 1 + base, dtype=dt).cuda()
    return gnnmp.GNNGraph(s, t, num_nodes=n, index_base=base)


def _np_edges(g):
    """1-based numpy (s, t) of a device graph"""
    return g.s.cpu().numpy().astype(np.int64) + (1 - g.index_base), g.t.cpu().numpy().astype(np.int64) + (1 - g.index_base)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["int32", "int64"])
@pytest.mark.parametrize("base", [0, 1])
@pytest.mark.parametrize("bidir", [True, False])
def test_negative_sample_properties(dtype, base, bidir):
    import torch
    import gnnmp
    rng = np.random.default_rng(3)
    n, m = 200, 1200
    s, t = rand_graph(n, m, bidir, rng)
    g = _graph(s, t, n, dtype, base)
    assert gnnmp.is_bidirected(g) == bidir
    num = 600
    gn = gnnmp.negative_sample(g, num_neg_edges=num, seed=11)          # bidirected = is_bidirected(g)
    assert gn.num_nodes == n and gn.index_base == base and gn.s.dtype == g.s.dtype and gn.w is None and gn.x is None
    assert gn.num_edges == num
    sn, tn = _np_edges(gn)
    half = num // 2 if bidir else num
    hs, ht = sn[:half], tn[:half]
    assert np.all((sn >= 1) & (sn <= n) & (tn >= 1) & (tn <= n))
    assert np.all(hs != ht)                                                       # no self loop
    assert not (edge_set(s, t) & edge_set(sn, tn))                                # no positive
    codes = (hs - 1) * n + ht
    assert len(np.unique(codes)) == half                                          # no duplicate code in the sampled half
    if bidir:
        assert np.array_equal(sn[half:], ht) and np.array_equal(tn[half:], hs)    # [s; t], [t; s]
        assert gnnmp.is_bidirected(gn)
    again = gnnmp.negative_sample(g, num_neg_edges=num, seed=11)
    assert torch.equal(again.s, gn.s) and torch.equal(again.t, gn.t)
    other = gnnmp.negative_sample(g, num_neg_edges=num, seed=12)
    assert not (torch.equal(other.s, gn.s) and torch.equal(other.t, gn.t))
    fresh = gnnmp.negative_sample(g, num_neg_edges=num)                           # seed = None: the module's sequence
    fresh2 = gnnmp.negative_sample(g, num_neg_edges=num)
    assert not torch.equal(fresh.s, fresh2.s)


@pytest.mark.gpu
def test_negative_sample_small_and_dense_cases():
    import gnnmp
    # dense: every non-edge but a few are positives; sample_prob = 1 and fewer edges than asked for come back
    n = 8
    allp = [(i, j) for i in range(1, n + 1) for j in range(1, n + 1) if i != j]
    keep = [e for k, e in enumerate(allp) if k % 7 != 0]
    s, t = np.array([e[0] for e in keep]), np.array([e[1] for e in keep])
    g = _graph(s, t, n)
    assert ref_sample_prob(n, len(s), 40) == 1.0
    gn = gnnmp.negative_sample(g, num_neg_edges=40, bidirected=False, seed=1)
    missing = sorted(set(allp) - set(keep))
    assert gn.num_edges == len(missing) < 40
    sn, tn = _np_edges(gn)
    assert list(zip(sn.tolist(), tn.tolist())) == missing          # p = 1: every non-positive code, ascending
    # n = 1: the only code is a self loop
    g1 = _graph(np.zeros(0, np.int64) + 1, np.zeros(0, np.int64) + 1, 1)
    assert gnnmp.negative_sample(g1, num_neg_edges=4, bidirected=False, seed=2).num_edges == 0
    # n = 0, num_neg_edges = 0
    g0 = _graph(np.zeros(0, np.int64), np.zeros(0, np.int64), 0)
    assert gnnmp.negative_sample(g0, num_neg_edges=0, bidirected=False).num_edges == 0
    assert gnnmp.negative_sample(g0, num_neg_edges=3, bidirected=True).num_edges == 0
    rng = np.random.default_rng(4)
    s, t = rand_graph(30, 60, True, rng)
    g = _graph(s, t, 30)
    gz = gnnmp.negative_sample(g, num_neg_edges=0, seed=3)
    assert gz.num_edges == 0 and gz.num_nodes == 30
    assert gnnmp.negative_sample(g, num_neg_edges=1, seed=3).num_edges == 0     # bidirected: 1 ÷ 2 = 0


@pytest.mark.gpu
@pytest.mark.parametrize("bidir", [True, False])
def test_negative_sample_distribution(bidir):
    """Inclusion frequency of every code over many seeds against the restatement's Monte-Carlo frequency.  The graph is dense enough
    that one trial usually falls short (pneg overestimates the non-edges) and the next ones overshoot: the union order and the
    truncation to the LOWEST codes of the last trial shape the distribution."""
    import gnnmp
    rng = np.random.default_rng(5)
    n = 16
    s, t = rand_graph(n, 100, bidir, rng)
    g = _graph(s, t, n)
    num = 40 if bidir else 30
    R, Rn = 3000, 20000
    f_dev = np.zeros(n * n)
    for r in range(R):
        gn = gnnmp.negative_sample(g, num_neg_edges=num, bidirected=bidir, seed=1000 + r)
        sn, tn = _np_edges(gn)
        half = len(sn) // 2 if bidir else len(sn)
        f_dev[(sn[:half] - 1) * n + tn[:half] - 1] += 1
    f_ref = np.zeros(n * n)
    lens = []
    for r in range(Rn):
        sn, tn = ref_negative_sample(s, t, n, num, bidir, rng)
        half = len(sn) // 2 if bidir else len(sn)
        lens.append(half)
        f_ref[(sn[:half] - 1) * n + tn[:half] - 1] += 1
    f_dev /= R
    f_ref /= Rn
    sigma = np.sqrt(f_ref * (1 - f_ref) * (1.0 / R + 1.0 / Rn))
    assert np.all(np.abs(f_dev - f_ref) <= 5 * sigma + 2e-3), np.max(np.abs(f_dev - f_ref) - 5 * sigma)
    # the trials reach the requested count almost always (the restatement's own sanity: the frequencies above are of full samples)
    assert np.mean(lens) > 0.9 * (num // 2 if bidir else num)


@pytest.mark.gpu
def test_negative_sample_products_scale():
    """ogbn-products' node count (n^2 = 6e12 codes) with 1e7 edges and num_neg = E: completes, exact count, no positive — the guard
    against any O(n^2) step"""
    import torch
    import gnnmp
    n, E = 2449029, 10_000_000
    gen = torch.Generator(device="cuda").manual_seed(7)
    s = torch.randint(1, n + 1, (E,), device="cuda", generator=gen)
    t = torch.randint(1, n + 1, (E,), device="cuda", generator=gen)
    g = gnnmp.GNNGraph(s, t, num_nodes=n)
    gn = gnnmp.negative_sample(g, num_neg_edges=E, bidirected=False, seed=9)
    assert gn.num_edges == E
    pos = torch.sort((s - 1) * n + (t - 1)).values
    neg = (gn.s - 1) * n + (gn.t - 1)
    at = torch.searchsorted(pos, neg).clamp(max=E - 1)
    assert not bool((pos[at] == neg).any())
    assert not bool((gn.s == gn.t).any())
    assert bool((torch.diff(neg) > 0).all())        # one trial: ascending, hence no duplicate


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["int32", "int64"])
@pytest.mark.parametrize("base", [0, 1])
def test_rand_edge_split(dtype, base):
    import torch
    import gnnmp
    rng = np.random.default_rng(6)
    n, m = 100, 300
    for bidir in (True, False):
        s, t = rand_graph(n, m, bidir, rng)
        g = _graph(s, t, n, dtype, base)
        g1, g2 = gnnmp.rand_edge_split(g, 0.9, seed=21)
        for h in (g1, g2):
            assert h.num_nodes == n and h.index_base == base and h.s.dtype == g.s.dtype and h.w is None
            assert gnnmp.is_bidirected(h) == bidir
        s1, t1 = _np_edges(g1)
        s2, t2 = _np_edges(g2)
        assert not (edge_set(s1, t1) & edge_set(s2, t2))
        assert g1.num_edges + g2.num_edges == m
        assert g2.num_edges < 50
        assert g1.num_edges == (2 * round(150 * 0.9) if bidir else round(300 * 0.9))
        # the two parts partition the edges
        assert sorted(zip(np.concatenate([s1, s2]).tolist(), np.concatenate([t1, t2]).tolist())) == sorted(zip(s.tolist(), t.tolist()))
        if bidir:   # a reverse pair never straddles the split; each part is [s; t], [t; s] over edges with s < t
            for a, b in ((s1, t1), (s2, t2)):
                h = len(a) // 2
                assert np.all(a[:h] < b[:h]) and np.array_equal(a[h:], b[:h]) and np.array_equal(b[h:], a[:h])
        again = gnnmp.rand_edge_split(g, 0.9, bidirected=bidir, seed=21)
        assert torch.equal(again[0].s, g1.s) and torch.equal(again[1].t, g2.t)
        other = gnnmp.rand_edge_split(g, 0.9, bidirected=bidir, seed=22)
        assert not torch.equal(other[0].s, g1.s)
    # round half to even: ne = 5, frac = 0.5 -> 2 edges in g1
    g = _graph(np.arange(1, 6), np.arange(2, 7), 6)
    g1, g2 = gnnmp.rand_edge_split(g, 0.5, bidirected=False, seed=1)
    assert (g1.num_edges, g2.num_edges) == (2, 3)
    assert gnnmp.rand_edge_split(g, 0.0, bidirected=False, seed=1)[0].num_edges == 0
    assert gnnmp.rand_edge_split(g, 1.0, bidirected=False, seed=1)[1].num_edges == 0
    with pytest.raises(IndexError):       # not bidirected: too few edges with s < t
        gnnmp.rand_edge_split(_graph(np.array([2, 3, 4, 5]), np.array([1, 2, 3, 4]), 5), 0.5, bidirected=True)


@pytest.mark.gpu
def test_rand_edge_split_is_uniform():
    """the permutation is uniform: every edge lands in g1 with probability size1 / ne, and its position is uniform"""
    import gnnmp
    ne = 12
    g = _graph(np.arange(1, ne + 1), np.arange(2, ne + 2), ne + 1)
    R = 3000
    cnt = np.zeros((ne, ne))
    for r in range(R):
        g1, _ = gnnmp.rand_edge_split(g, 1.0, bidirected=False, seed=r)
        s1, _ = _np_edges(g1)
        cnt[np.arange(ne), s1 - 1] += 1            # position i holds edge s1[i]
    f = cnt / R
    sigma = np.sqrt((1 / ne) * (1 - 1 / ne) / R)
    assert np.all(np.abs(f - 1 / ne) <= 5 * sigma)


# ---------------------------------------------------------------------------------------------------------
# the adjoint of the per-edge dot product
# ---------------------------------------------------------------------------------------------------------
def _adjoint_graph(n, rng):
    """hub rows (a node with many in- and out-edges), self loops, empty rows (isolated nodes), a multi-edge"""
    E = 6 * n
    s = rng.integers(0, n - 5, E)
    t = rng.integers(0, n - 5, E)
    hub_in = np.full(3000, 3)
    hub_out_t = rng.integers(0, n - 5, 2500)
    s = np.concatenate([s, rng.integers(0, n - 5, 3000), np.full(2500, 7), [10, 11, 12, 12, 9, 9]])
    t = np.concatenate([t, hub_in, hub_out_t, [10, 11, 12, 12, 4, 4]])
    return s + 1, t + 1          # nodes n-5 .. n-1 have no edge at all


def _close(got, ref, tol=1e-5):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape
    assert np.linalg.norm(got - ref) <= tol * np.linalg.norm(ref)
    assert np.abs(got - ref).max() <= tol * max(np.abs(ref).max(), 1e-30)


def _np_grads(s, t, xi, xj, dz):
    s0, t0 = s - 1, t - 1
    xi64, xj64, dz64 = xi.astype(np.float64), xj.astype(np.float64), dz.astype(np.float64)
    dxi = np.zeros_like(xi64)
    dxj = np.zeros_like(xj64)
    np.add.at(dxi, t0, dz64[:, None] * xj64[s0])
    np.add.at(dxj, s0, dz64[:, None] * xi64[t0])
    return dxi, dxj


@pytest.mark.gpu
@pytest.mark.parametrize("D", [1, 7, 64, 256, 300])
def test_edge_dot_grad(D):
    import torch
    import gnnmp
    from gnnmp import _lib
    rng = np.random.default_rng(D)
    n = 1500
    s, t = _adjoint_graph(n, rng)
    g = _graph(s, t, n)
    xi = rng.standard_normal((n, D)).astype(np.float32)
    xj = rng.standard_normal((n, D)).astype(np.float32)
    dz = rng.standard_normal(len(s)).astype(np.float32)
    Xi, Xj, Dz = (torch.from_numpy(a).cuda() for a in (xi, xj, dz))
    ri, rj = _np_grads(s, t, xi, xj, dz)
    dxi, dxj = gnnmp.edge_dot_grad(g, Xi, Xj, Dz)
    _close(dxi.cpu().numpy(), ri)
    _close(dxj.cpu().numpy(), rj)
    dxa, none = gnnmp.edge_dot_grad(g, Xi, Xi, Dz, alias=True)
    assert none is None
    ra = sum(_np_grads(s, t, xi, xi, dz))
    _close(dxa.cpu().numpy(), ra)
    # reruns are bit-identical
    dxi2, dxj2 = gnnmp.edge_dot_grad(g, Xi, Xj, Dz)
    assert torch.equal(dxi, dxi2) and torch.equal(dxj, dxj2)
    assert torch.equal(dxa, gnnmp.edge_dot_grad(g, Xi, Xi, Dz, alias=True)[0])
    # the fused kernel agrees with the composition of two propagates (knob 21 < 0: the A/B baseline)
    with _lib.tuned(_lib.Knob.EDGE_DOT_GRAD, -1):
        ci, cj = gnnmp.edge_dot_grad(g, Xi, Xj, Dz)
        ca, _ = gnnmp.edge_dot_grad(g, Xi, Xi, Dz, alias=True)
    # same products, same edge order: bit-identical on the rows the propagate does not split, the hub rows (folded chunk by chunk
    # there) within the float32 reordering of a 3000-term sum
    short_in, short_out = np.bincount(t - 1, minlength=n) <= 64, np.bincount(s - 1, minlength=n) <= 64
    assert np.array_equal(ci.cpu().numpy()[short_in], dxi.cpu().numpy()[short_in])
    assert np.array_equal(cj.cpu().numpy()[short_out], dxj.cpu().numpy()[short_out])
    _close(ci.cpu().numpy(), ri)
    _close(cj.cpu().numpy(), rj)
    _close(ca.cpu().numpy(), ra)
    # the C entry point itself: D > 256 is refused, the caller composes
    rc = _lib.load().gnnmp_edge_dot_grad_f32(g.plan(False).handle, g.plan_transposed(False).handle, _lib.ptr(Xi), _lib.ptr(Xj),
                                             _lib.ptr(Dz), _lib.ptr(dxi), _lib.ptr(dxj), D, _lib.stream_ptr())
    assert rc == (_lib.EUNSUPPORTED if D > 256 else _lib.OK)
    rc = _lib.load().gnnmp_edge_dot_grad_f32(g.plan(True).handle, g.plan_transposed(True).handle, _lib.ptr(Xi), _lib.ptr(Xj),
                                             _lib.ptr(Dz), _lib.ptr(dxi), _lib.ptr(dxj), min(D, 256), _lib.stream_ptr())
    assert rc == _lib.EINVAL


@pytest.mark.gpu
def test_dot_decoder_autograd():
    import torch
    import gnnmp
    rng = np.random.default_rng(8)
    n, D = 400, 33
    s, t = _adjoint_graph(n, rng)
    g = _graph(s, t, n)
    x = rng.standard_normal((n, D)).astype(np.float32)
    y = rng.standard_normal((n, D)).astype(np.float32)
    dz = rng.standard_normal(len(s)).astype(np.float32)
    X = torch.from_numpy(x).cuda().requires_grad_(True)
    Y = torch.from_numpy(y).cuda().requires_grad_(True)
    z = gnnmp.dot_decoder_ad(g, X)
    assert z.shape == (len(s), 1)
    zr = np.sum(x[t - 1].astype(np.float64) * x[s - 1], axis=1, keepdims=True)
    _close(z.detach().cpu().numpy(), zr)
    (z[:, 0] * torch.from_numpy(dz).cuda()).sum().backward()
    _close(X.grad.cpu().numpy(), sum(_np_grads(s, t, x, x, dz)))
    X.grad = None
    z2 = gnnmp.edge_dot_ad(g, X, Y)
    (z2[:, 0] * torch.from_numpy(dz).cuda()).sum().backward()
    ri, rj = _np_grads(s, t, x, y, dz)
    _close(X.grad.cpu().numpy(), ri)
    _close(Y.grad.cpu().numpy(), rj)
    # DotDecoder is a graph layer: it closes a GNNChain
    chain = gnnmp.GNNChain(gnnmp.GCNConv((D, 16), "relu", seed=1), gnnmp.DotDecoder())
    out = chain(g, X.detach())
    h = chain.layers[0](g, X.detach())
    assert out.shape == (len(s), 1)
    assert torch.equal(out, gnnmp.apply_edges(gnnmp.xi_dot_xj, g, xi=h, xj=h))
    wg = gnnmp.WithGraph(chain, g)
    assert torch.equal(wg(X.detach()), out) and torch.equal(wg(g, X.detach()), out)


# ---------------------------------------------------------------------------------------------------------
# the example's training loop, end to end
# ---------------------------------------------------------------------------------------------------------
def planted_links(seed=0, n=19717, E=88648, D=500, k=40):
    """a PubMed-shaped bidirected graph (n nodes, E directed edges, D features) whose edges mostly join nodes of one of k hidden
    communities; the features carry a noisy copy of the community"""
    rng = np.random.default_rng(seed)
    comm = rng.integers(0, k, n)
    order = np.argsort(comm, kind="stable")
    starts = np.searchsorted(comm[order], np.arange(k))
    ends = np.append(starts[1:], n)
    m = E // 2
    a = rng.integers(0, n, 2 * m)
    inside = rng.random(2 * m) < 0.9
    b_in = order[starts[comm[a]] + (rng.random(2 * m) * (ends[comm[a]] - starts[comm[a]])).astype(np.int64)]
    b = np.where(inside, b_in, rng.integers(0, n, 2 * m))
    u, v = np.minimum(a, b), np.maximum(a, b)
    keep = u != v
    pairs = np.unique(u[keep] * n + v[keep])[:m]
    rng.shuffle(pairs)
    u, v = pairs // n, pairs % n
    s = np.concatenate([u, v]) + 1
    t = np.concatenate([v, u]) + 1
    centres = rng.standard_normal((k, D)).astype(np.float32)
    x = (1.0 * centres[comm] + rng.standard_normal((n, D))).astype(np.float32)
    return s, t, x


@pytest.mark.gpu
def test_link_prediction_training_learns():
    """link_prediction_pubmed.jl: rand_edge_split(0.9), GCNConv(500 => 64, relu) -> GCNConv(64 => 64) on the training edges, DotDecoder
    on the positive and a freshly sampled negative graph every step, logit BCE; test accuracy on the held-out edges and a fixed
    negative sample well above chance"""
    import torch
    import torch.nn.functional as F
    import gnnmp
    from gnnmp.backward import gcn_conv_ad
    s, t, x = planted_links()
    n, D = x.shape
    g = gnnmp.GNNGraph(torch.from_numpy(s).cuda(), torch.from_numpy(t).cuda(), num_nodes=n)
    X = torch.from_numpy(x).cuda()
    assert gnnmp.is_bidirected(g)
    train_pos, test_pos = gnnmp.rand_edge_split(g, 0.9, seed=17)
    test_neg = gnnmp.negative_sample(g, num_neg_edges=test_pos.num_edges, seed=18)
    l1, l2 = gnnmp.GCNConv((D, 64), "relu", seed=1), gnnmp.GCNConv((64, 64), None, seed=2)
    params = [l1.weight, l1.bias, l2.weight, l2.bias]
    for p in params:
        p.requires_grad_(True)
    opt = torch.optim.Adam(params, lr=1e-2)
    model = gnnmp.WithGraph(lambda gg, h: gcn_conv_ad(l2, gg, gcn_conv_ad(l1, gg, h)), train_pos)

    def loss(pos_g, neg_g=None):
        h = model(X)
        if neg_g is None:
            neg_g = gnnmp.negative_sample(pos_g, bidirected=True)    # a fresh negative graph every step, on the device
        ps, ns = gnnmp.dot_decoder_ad(pos_g, h)[:, 0], gnnmp.dot_decoder_ad(neg_g, h)[:, 0]
        scores = torch.cat([ps, ns])
        labels = torch.cat([torch.ones_like(ps), torch.zeros_like(ns)])
        acc = 0.5 * float((ps >= 0).float().mean()) + 0.5 * float((ns < 0).float().mean())
        return F.binary_cross_entropy_with_logits(scores, labels), acc

    with torch.no_grad():
        _, acc0 = loss(test_pos, test_neg)
    losses = []
    for step in range(60):
        opt.zero_grad()
        l, _ = loss(train_pos)
        l.backward()
        opt.step()
        losses.append(float(l.detach()))
    with torch.no_grad():
        _, acc = loss(test_pos, test_neg)
    assert np.isfinite(losses).all()
    assert losses[-1] < 0.7 * losses[0], (losses[0], losses[-1])
    assert acc > 0.65, (acc0, acc)
