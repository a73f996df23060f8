"""remove_nodes / add_edges / add_nodes / perturb_edges on DERIVED plans (csrc/plan_edit.hip, gnnmp/transform.py), on the device:
  gnnmp_plan_remove_nodes / gnnmp_plan_add_edges   the child's plan written from the parent's without a sort — bit-identical (rowptr, col,
                                                   eid, gnnmp_plan_info but the bytes held) to gnnmp_plan_create on the child's COO as
                                                   tests/augment_ref.py restates it, for plain, self-looped and transposed parents
  their memory contract                            (both are lifecycle calls, outside the case table of tests/abi_cases.py): outputs written
                                                   in exactly the promised prefix, nothing past it, inputs and the parent plan untouched
  the Python mirror                                the four transforms against augment_ref on a weighted batch with features
The header and refusal tests, which need no device, are in tests/test_augment.py.  This file sorts behind tests/test_placement.py on
purpose: the placement arena finds its classes by where hipMalloc happens to put 2 GiB blocks, which depends on every allocation the
process made before, so the many small plan builds here run after it."""
import ctypes
import itertools

import numpy as np
import pytest

import augment_ref as R

LONG_ROW, MIN_LONG_ROW = 512, 64


# ---- on the device --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gm():
    import torch
    assert torch.cuda.is_available()
    import gnnmp
    gnnmp.load()
    return gnnmp


def _dev(a, dt):
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(dt))).cuda()


def _plan(s0, t0, n, base, ib, loops, transposed):
    """gnnmp_plan_create on 0-based numpy (s0, t0), handed over in (ib, base)"""
    from gnnmp.graph import Plan
    dt = np.int64 if ib == 8 else np.int32
    a, b = (t0, s0) if transposed else (s0, t0)
    return Plan(_dev(np.asarray(a) + base, dt), _dev(np.asarray(b) + base, dt), n, n, base, loops, validate=True)


INFO = ("n_src", "n_dst", "n_edges", "n_total", "max_degree", "n_long", "long_thresh")


def _same(p, q, tag):
    for f in INFO:                                                       # gnnmp_plan_info, all but the bytes held
        assert getattr(p, f) == getattr(q, f), f"{tag}: {f} {getattr(p, f)} != {getattr(q, f)}"
    for name, a, b in zip(("rowptr", "col", "eid"), p.export(), q.export()):
        assert np.array_equal(a.cpu().numpy(), b.cpu().numpy()), f"{tag}: {name} differs"


def _remove(parent, lst, ib, base, p=0.0, seed=0, maps=None):
    from gnnmp import _lib as L
    from gnnmp.graph import Plan
    h, tot = ctypes.c_void_p(), (ctypes.c_int64 * 2)()
    nm, nn, em = maps if maps is not None else (None, None, None)
    rc = L.load().gnnmp_plan_remove_nodes(ctypes.byref(h), parent.handle, L.ptr(lst), ib, base, 0 if lst is None else lst.numel(), p,
                                          ctypes.c_uint64(seed), L.ptr(nm), L.ptr(nn), L.ptr(em), tot, L.stream_ptr())
    L.check(rc)
    return Plan._adopt(h, parent.device), tot[0], tot[1]


def _add(parent, s, t, ib, base, m, n_nodes, seed=0, outs=(None, None)):
    from gnnmp import _lib as L
    from gnnmp.graph import Plan
    h = ctypes.c_void_p()
    L.check(L.load().gnnmp_plan_add_edges(ctypes.byref(h), parent.handle, L.ptr(s), L.ptr(t), ib, base, m, n_nodes, ctypes.c_uint64(seed),
                                          L.ptr(outs[0]), L.ptr(outs[1]), L.stream_ptr()))
    return Plan._adopt(h, parent.device)


def _hub_graph(rng, N=700, hub=5, fan=600, extra=400):
    """node `hub` with `fan` in-edges from the distinct sources 100 .. 100 + fan - 1, among `extra` random edges"""
    s = np.concatenate([rng.integers(0, N, extra), np.arange(100, 100 + fan)])
    t = np.concatenate([rng.integers(0, N, extra), np.full(fan, hub)])
    perm = rng.permutation(len(s))
    return s[perm], t[perm], N


def _graphs():
    """name -> (s0, t0, N): the shapes of the issue — N, E at 31 / 33 / 300, one past the scan's 4096-element block, several blocks"""
    rng = np.random.default_rng(2024)
    out = {"n1_e0": (np.zeros(0, np.int64), np.zeros(0, np.int64), 1), "n33_e0": (np.zeros(0, np.int64), np.zeros(0, np.int64), 33)}
    for n, e in ((31, 33), (33, 31), (300, 300), (4097, 4097), (5000, 70001)):
        out[f"n{n}_e{e}"] = (rng.integers(0, n, e), rng.integers(0, n, e), n)
    out["hub"] = _hub_graph(rng)
    return out


GRAPHS = _graphs()
KINDS = list(itertools.product((False, True), (False, True)))        # (self loops, transposed)
WIRE = [(4, 0), (8, 1), (4, 1), (8, 0)]                              # (idx_bytes, index_base)


def _remove_lists(name, s0, t0, N, rng):
    """what to remove: nothing, everything, a descending list with repeats, the two hub cuts"""
    yield "none", np.zeros(0, np.int64)
    yield "all", np.arange(N)
    pick = rng.choice(N, max(1, N // 3), replace=False)
    yield "desc_dups", np.sort(np.concatenate([pick, pick[: max(1, len(pick) // 2)]]))[::-1]
    if name == "hub":
        yield "hub_stays_long", np.arange(100, 120)                   # 580 of the hub's 600 in-edges stay: above GNNMP_LONG_ROW
        yield "hub_cut_short", np.arange(150, 700)                    # 50 stay (+ a few random ones): below GNNMP_MIN_LONG_ROW


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(GRAPHS))
def test_remove_nodes_plan_is_plan_create_on_the_child_coo(gm, name):
    import torch
    s0, t0, N = GRAPHS[name]
    rng = np.random.default_rng(len(name) + N)
    lists = [(what, lst, R.remove_nodes(s0, t0, None, N, lst, base=0)) for what, lst in _remove_lists(name, s0, t0, N, rng)]
    for (ib, base), (loops, tr) in itertools.product(WIRE, KINDS):
        dt = np.int64 if ib == 8 else np.int32
        parent = _plan(s0, t0, N, base, ib, loops, tr)
        for what, lst, (s2, t2, _, n2, nid, eid) in lists:
            tag = f"{name} {what} ib{ib} base{base} loops{loops} T{tr}"
            lst_dev = _dev(lst + base, dt) if len(lst) else None
            nm = torch.full((N,), -7, dtype=torch.int32, device="cuda")
            nn = torch.full((N,), -7, dtype=torch.int32, device="cuda")
            em = torch.full((max(len(s0), 1),), -7, dtype=torch.int32, device="cuda")
            child, nk, ek = _remove(parent, lst_dev, ib, base, maps=(nm, nn, em))
            assert (nk, ek) == (n2, len(s2)), tag
            _same(child, _plan(s2, t2, n2, base, ib, loops, tr), tag)
            assert np.array_equal(nm[:nk].cpu().numpy(), nid) and np.array_equal(em[:ek].cpu().numpy(), eid), tag
            new = np.full(N, -1)
            new[nid] = np.arange(n2)
            assert np.array_equal(nn.cpu().numpy(), new), tag
            if name == "hub" and not loops and not tr:
                ref = _plan(s2, t2, n2, base, ib, loops, tr)
                if what == "hub_stays_long":
                    assert child.max_degree > LONG_ROW and child.n_long >= 1
                if what == "hub_cut_short":
                    assert child.max_degree < MIN_LONG_ROW and child.n_long == 0 and parent.n_long >= 1
                x = torch.randn((n2, 12), device="cuda")
                ga = gm.GNNGraph._from_plan(child, 1, None, None, base, torch.int64)
                gb = gm.GNNGraph._from_plan(ref, 1, None, None, base, torch.int64)
                assert torch.equal(gm.propagate(gm.copy_xj, ga, "+", xj=x), gm.propagate(gm.copy_xj, gb, "+", xj=x)), tag


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["n33_e0", "n300_e300", "n4097_e4097", "hub"])
def test_remove_nodes_random_mode_is_the_dropout_mask(gm, name):
    s0, t0, N = GRAPHS[name]
    for k, p in enumerate((0.0, 0.3, 0.5, 1.0)):
        seed = 0xDEADBEEF12345 + k
        ib, base = WIRE[k]
        loops, tr = KINDS[k]
        s2, t2, _, n2, nid, eid = R.remove_nodes_p(s0, t0, None, N, p, seed, base=0)
        assert (p > 0.0 or n2 == N) and (p < 1.0 or n2 == 0)
        child, nk, ek = _remove(_plan(s0, t0, N, base, ib, loops, tr), None, ib, base, p=p, seed=seed)
        assert (nk, ek) == (n2, len(s2))
        _same(child, _plan(s2, t2, n2, base, ib, loops, tr), f"{name} p{p}")


def _new_edges(name, s0, t0, N, rng):
    """(what, s_new, t_new, n_nodes): one edge, more than E, all on one row, new nodes with and without edges"""
    E = len(s0)
    yield "m1", rng.integers(0, N, 1), rng.integers(0, N, 1), N
    m = E + 7
    yield "m_gt_E", rng.integers(0, N, m), rng.integers(0, N, m), N
    yield "one_row", rng.integers(0, N, 70), np.full(70, N // 2), N
    yield "new_nodes_only", np.zeros(0, np.int64), np.zeros(0, np.int64), N + 9
    yield "into_new_nodes", rng.integers(0, N + 5, 40), rng.integers(0, N + 5, 40), N + 5
    if name == "hub":
        yield "hub_grows", rng.integers(0, N, 100), np.full(100, 5), N


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(GRAPHS))
def test_add_edges_plan_is_plan_create_on_the_child_coo(gm, name):
    import torch
    s0, t0, N = GRAPHS[name]
    rng = np.random.default_rng(7 * len(name) + N)
    cases = list(_new_edges(name, s0, t0, N, rng))
    for (ib, base), (loops, tr) in itertools.product(WIRE, KINDS):
        dt = np.int64 if ib == 8 else np.int32
        parent = _plan(s0, t0, N, base, ib, loops, tr)
        for what, sn, tn, n_nodes in cases:
            tag = f"{name} {what} ib{ib} base{base} loops{loops} T{tr}"
            s2, t2 = np.concatenate([s0, sn]), np.concatenate([t0, tn])
            a, b = (tn, sn) if tr else (sn, tn)                         # the pair swapped derives the transposed child
            sd, td = (_dev(a + base, dt), _dev(b + base, dt)) if len(sn) else (None, None)
            child = _add(parent, sd, td, ib, base, len(sn), n_nodes)
            ref = _plan(s2, t2, n_nodes, base, ib, loops, tr)
            _same(child, ref, tag)
            if name == "hub" and not loops and not tr:
                x = torch.randn((n_nodes, 12), device="cuda")
                ga = gm.GNNGraph._from_plan(child, 1, None, None, base, torch.int64)
                gb = gm.GNNGraph._from_plan(ref, 1, None, None, base, torch.int64)
                assert child.n_long >= 1
                assert torch.equal(gm.propagate(gm.copy_xj, ga, "+", xj=x), gm.propagate(gm.copy_xj, gb, "+", xj=x)), tag


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["n31_e33", "n300_e300", "n5000_e70001"])
def test_add_edges_random_mode_is_the_restated_pair_draw(gm, name):
    import torch
    s0, t0, N = GRAPHS[name]
    for k, m in enumerate((1, 33, len(s0) + 1, 4097)):
        seed = (k << 40) + 99
        ib, base = WIRE[k]
        loops, tr = bool(k & 1), False         # (a transposed child takes the drawn pairs in list mode, swapped: the test above)
        tdt = torch.int64 if ib == 8 else torch.int32
        sn, tn = R.rand_pairs(seed, m, N)
        so, to = torch.full((m,), -7, dtype=tdt, device="cuda"), torch.full((m,), -7, dtype=tdt, device="cuda")
        child = _add(_plan(s0, t0, N, base, ib, loops, tr), None, None, ib, base, m, N, seed=seed, outs=(so, to))
        assert np.array_equal(so.cpu().numpy(), sn + base) and np.array_equal(to.cpu().numpy(), tn + base)
        _same(child, _plan(np.concatenate([s0, sn]), np.concatenate([t0, tn]), N, base, ib, loops, tr), f"{name} m{m}")


@pytest.mark.gpu
def test_device_side_bounds_checks(gm):
    from gnnmp import _lib as L
    s0, t0, N = GRAPHS["n31_e33"]
    parent = _plan(s0, t0, N, 1, 8, False, False)
    with pytest.raises(L.GnnmpError) as e:
        _remove(parent, _dev([3, N + 1], np.int64), 8, 1)
    assert e.value.status == L.EBOUNDS
    with pytest.raises(L.GnnmpError) as e:
        _remove(parent, _dev([0], np.int64), 8, 1)
    assert e.value.status == L.EBOUNDS
    with pytest.raises(L.GnnmpError) as e:
        _add(parent, _dev([1, 2], np.int64), _dev([2, N + 3], np.int64), 8, 1, 2, N + 2)
    assert e.value.status == L.EBOUNDS
    with pytest.raises(L.GnnmpError) as e:
        _add(parent, _dev([0], np.int64), _dev([2], np.int64), 8, 1, 1, N)
    assert e.value.status == L.EBOUNDS
    _same(_remove(parent, None, 8, 1)[0], parent, "the parent still works")


# ---- the memory contract ----------------------------------------------------------------------------------------------------------
POISON32 = 0x5A5A5A5A
GUARD = 64      # int32 words between and around the carved outputs


class _Carver:
    """outputs carved from ONE poisoned int32 buffer, guard bands between them, every start element-aligned but off the 16-byte grid"""

    def __init__(self, words):
        import torch
        self.buf = torch.full((words,), POISON32, dtype=torch.int32, device="cuda")
        self.at, self.taken = GUARD, []

    def take(self, n, elem_words, promised):
        off = (self.at + 3) // 4 * 4 + elem_words            # 16-byte boundary + one element: aligned to the element only
        self.at = off + n * elem_words + GUARD
        assert self.at <= self.buf.numel()
        self.taken.append((off, n * elem_words, promised * elem_words))
        assert (self.buf.data_ptr() + 4 * off) % 16 != 0 and (self.buf.data_ptr() + 4 * off) % (4 * elem_words) == 0
        return ctypes.c_void_p(self.buf.data_ptr() + 4 * off), off

    def read(self, off, n, dt):
        return self.buf[off: off + n * (2 if dt == np.int64 else 1)].cpu().numpy().view(dt)

    def check(self, tag):
        host = self.buf.cpu().numpy()
        mask = np.ones(host.size, bool)
        for off, cap, promised in self.taken:
            mask[off: off + promised] = False
        assert np.all(host[mask] == POISON32), f"{tag}: a word outside the promised prefixes was written"


@pytest.mark.gpu
@pytest.mark.parametrize("side", [False, True])
@pytest.mark.parametrize("ib,base", [(4, 0), (8, 1)])
def test_memory_contract_of_remove_nodes(gm, ib, base, side):
    import torch
    from gnnmp import _lib as L
    from gnnmp.graph import Plan
    s0, t0, N = GRAPHS["n300_e300"]
    E = len(s0)
    dt = np.int64 if ib == 8 else np.int32
    lst = np.array([299, 7, 7, 150, 12, 0, 299])
    s2, t2, _, n2, nid, eid = R.remove_nodes(s0, t0, None, N, lst, base=0)
    stream = torch.cuda.Stream() if side else torch.cuda.current_stream()
    with torch.cuda.stream(stream):
        parent = _plan(s0, t0, N, base, ib, True, False)
        before = [a.clone() for a in parent.export()]
        lst_dev = _dev(lst + base, dt)
        lst_copy = lst_dev.clone()
        cv = _Carver(4 * N + 2 * E + 16 * GUARD)
        (nm, o_nm), (nn, o_nn), (em, o_em) = cv.take(N, 1, n2), cv.take(N, 1, N), cv.take(E, 1, len(s2))
        h, tot = ctypes.c_void_p(), (ctypes.c_int64 * 2)()
        L.check(L.load().gnnmp_plan_remove_nodes(ctypes.byref(h), parent.handle, L.ptr(lst_dev), ib, base, len(lst), 0.0, 0, nm, nn, em,
                                                 tot, L.stream_ptr()))
        child = Plan._adopt(h, parent.device)
        assert (tot[0], tot[1]) == (n2, len(s2))
        assert np.array_equal(cv.read(o_nm, n2, np.int32), nid) and np.array_equal(cv.read(o_em, len(s2), np.int32), eid)
        new = np.full(N, -1)
        new[nid] = np.arange(n2)
        assert np.array_equal(cv.read(o_nn, N, np.int32), new)              # written whole
        cv.check(f"remove_nodes ib{ib}")
        assert torch.equal(lst_dev, lst_copy)
        for a, b in zip(before, parent.export()):
            assert torch.equal(a, b)
        _same(child, _plan(s2, t2, n2, base, ib, True, False), "carved outputs")
        # NULL outputs: the same plan, nothing else touched
        _same(_remove(parent, lst_dev, ib, base)[0], child, "NULL outputs")
    stream.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("side", [False, True])
@pytest.mark.parametrize("ib,base", [(4, 0), (8, 1)])
def test_memory_contract_of_add_edges(gm, ib, base, side):
    import torch
    from gnnmp import _lib as L
    from gnnmp.graph import Plan
    s0, t0, N = GRAPHS["n300_e300"]
    dt = np.int64 if ib == 8 else np.int32
    m, seed, ew = 77, 0x1234567890, ib // 4
    sn, tn = R.rand_pairs(seed, m, N)
    s2, t2 = np.concatenate([s0, sn]), np.concatenate([t0, tn])
    stream = torch.cuda.Stream() if side else torch.cuda.current_stream()
    with torch.cuda.stream(stream):
        parent = _plan(s0, t0, N, base, ib, True, False)
        before = [a.clone() for a in parent.export()]
        cv = _Carver(4 * m * ew + 16 * GUARD)
        (so, o_s), (to, o_t) = cv.take(m + 5, ew, m), cv.take(m + 5, ew, m)       # room for 5 more: only m entries are promised
        h = ctypes.c_void_p()
        L.check(L.load().gnnmp_plan_add_edges(ctypes.byref(h), parent.handle, None, None, ib, base, m, N + 3, ctypes.c_uint64(seed), so, to,
                                              L.stream_ptr()))
        child = Plan._adopt(h, parent.device)
        assert np.array_equal(cv.read(o_s, m, dt), sn + base) and np.array_equal(cv.read(o_t, m, dt), tn + base)
        cv.check(f"add_edges ib{ib}")
        ref = _plan(s2, t2, N + 3, base, ib, True, False)
        _same(child, ref, "random mode")
        # list mode on element-aligned inputs off the 16-byte grid: inputs come back bit for bit, the outputs are not touched
        pad = torch.full((2 * (m + 8),), -3, dtype=torch.int64 if ib == 8 else torch.int32, device="cuda")
        pad[1: m + 1] = _dev(sn + base, dt)
        pad[m + 8 + 1: m + 8 + 1 + m] = _dev(tn + base, dt)
        copy = pad.clone()
        cv2 = _Carver(4 * m * ew + 16 * GUARD)
        (so2, _), (to2, _) = cv2.take(m, ew, 0), cv2.take(m, ew, 0)
        h2 = ctypes.c_void_p()
        es = pad.element_size()
        L.check(L.load().gnnmp_plan_add_edges(ctypes.byref(h2), parent.handle, ctypes.c_void_p(pad.data_ptr() + es),
                                              ctypes.c_void_p(pad.data_ptr() + es * (m + 9)), ib, base, m, N + 3, 0, so2, to2,
                                              L.stream_ptr()))
        _same(Plan._adopt(h2, parent.device), ref, "list mode, unaligned inputs")
        cv2.check("add_edges list mode")
        assert torch.equal(pad, copy)
        for a, b in zip(before, parent.export()):
            assert torch.equal(a, b)
    stream.synchronize()


# ---- the Python mirror ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def batch3(gm):
    """a weighted batch of three small graphs with x, edata and a graph indicator (1-based int64, like the reference)"""
    import torch
    rng = np.random.default_rng(31)
    gs, ms = [], []
    for n, e in ((7, 15), (12, 30), (9, 0)):
        s, t = rng.integers(1, n + 1, e), rng.integers(1, n + 1, e)
        w = rng.random(e).astype(np.float32)
        x = rng.standard_normal((n, 5)).astype(np.float32)
        gs.append(gm.GNNGraph(_dev(s, np.int64), _dev(t, np.int64), torch.from_numpy(w).cuda(), num_nodes=n, x=torch.from_numpy(x).cuda()))
        ms.append((s, t, w, x, n))
    g = gm.batch(gs)
    off = np.cumsum([0] + [m[4] for m in ms])
    s = np.concatenate([m[0] + o for m, o in zip(ms, off)])
    t = np.concatenate([m[1] + o for m, o in zip(ms, off)])
    w = np.concatenate([m[2] for m in ms])
    x = np.concatenate([m[3] for m in ms])
    gi = np.concatenate([np.full(m[4], k + 1) for k, m in enumerate(ms)])
    edata = {"e": torch.from_numpy(rng.standard_normal((len(s), 3)).astype(np.float32)).cuda()}
    assert np.array_equal(g.s.cpu().numpy(), s) and np.array_equal(g.graph_indicator.cpu().numpy(), gi)
    return g, dict(s=s, t=t, w=w, x=x, gi=gi, n=int(off[-1]), edata=edata)


def _np(v):
    return v.cpu().numpy()


def _is_graph(g2, s, t, w, n):
    assert (g2.num_nodes, g2.num_edges) == (n, len(s))
    assert np.array_equal(_np(g2.s), s) and np.array_equal(_np(g2.t), t)
    assert (g2.w is None) == (w is None) and (w is None or np.array_equal(_np(g2.w), np.asarray(w, np.float32)))


def _conv_bits(gm, g2, x):
    """gcn_conv and graph_conv_ad (forward + the three gradients) on g2"""
    import torch
    from gnnmp.backward import graph_conv_ad
    out = [gm.gcn_conv(gm.GCNConv((x.shape[1], 6), "relu", seed=3), g2, x)]
    l = gm.GraphConv((x.shape[1], 4), "relu", seed=4)
    xt = x.clone().requires_grad_(True)
    for v in (l.weight1, l.weight2, l.bias):
        v.requires_grad_(True)
    y = graph_conv_ad(l, g2, xt)
    y.sum().backward()
    return out + [y.detach(), xt.grad, l.weight1.grad, l.weight2.grad, l.bias.grad]


def _derived_equals_built(gm, parent, make):
    """the child's convolutions give the same bits whether its plans were derived from the parent's or built from its own COO"""
    import torch
    for key in (True, False):
        parent.plan(key), parent.plan_transposed(key)
    child = make()
    x = child.x if child.x is not None else torch.randn((child.num_nodes, 5), device="cuda")
    derived = _conv_bits(gm, child, x)
    # every plan the convolutions asked for was derived (a pooled plan), none built from the child's COO
    assert len(child._plans) >= 2 and all(getattr(q, "_pooled", False) for q in child._plans.values()), list(child._plans)
    built = gm.GNNGraph(child.s, child.t, child.w, num_nodes=child.num_nodes, x=child.x, graph_indicator=child.graph_indicator,
                        num_graphs=child.num_graphs)
    for k in (False, True):
        _same(child.plan(k), built.plan(k), f"plan({k})")
        _same(child.plan_transposed(k), built.plan_transposed(k), f"plan_transposed({k})")
    for a, b in zip(derived, _conv_bits(gm, built, x)):
        assert torch.equal(a, b)


@pytest.mark.gpu
def test_python_remove_nodes(gm, batch3):
    import torch
    g, h = batch3
    nodes = [20, 3, 3, 28, 1]
    s2, t2, w2, n2, nid, eid = R.remove_nodes(h["s"], h["t"], h["w"], h["n"], nodes)
    g2, ed2 = gm.remove_nodes(g, nodes, edata=h["edata"])
    _is_graph(g2, s2, t2, w2, n2)
    assert np.array_equal(_np(g2.nid), nid + 1) and np.array_equal(_np(g2.eid), eid + 1) and g2.nid.dtype == g.s.dtype
    assert np.array_equal(_np(g2.x), h["x"][nid]) and np.array_equal(_np(ed2["e"]), _np(h["edata"]["e"])[eid])
    assert np.array_equal(_np(g2.graph_indicator), h["gi"][nid]) and g2.num_graphs == 3          # the documented deviation
    assert gm.remove_nodes(g, torch.tensor(nodes)).num_nodes == n2 and isinstance(gm.remove_nodes(g, nodes), gm.GNNGraph)
    # random: the list call on the mask's zeros; same seed same graph, another seed another graph
    seed, p = 1234, 0.4
    from gnnmp.layers import dropout_keep
    keep = _np(dropout_keep(seed, p, g.num_nodes, 1)).reshape(-1)
    a, b = gm.remove_nodes(g, p, seed=seed), gm.remove_nodes(g, (np.flatnonzero(keep == 0) + 1).tolist())
    assert 0 < a.num_nodes < g.num_nodes
    _is_graph(a, _np(b.s), _np(b.t), _np(b.w), b.num_nodes)
    assert torch.equal(a.nid, b.nid) and torch.equal(a.eid, b.eid) and torch.equal(a.x, b.x)
    assert torch.equal(gm.remove_nodes(g, p, seed=seed).nid, a.nid)
    assert not torch.equal(gm.remove_nodes(g, p, seed=seed + 1).nid, a.nid)
    assert gm.remove_nodes(g, 0.0).num_nodes == g.num_nodes and gm.remove_nodes(g, 1.0).num_nodes == 0
    assert gm.remove_nodes(g, 1.0).num_edges == 0 and gm.remove_nodes(g, 1.0).x.shape == (0, 5)
    for bad in ([0], [29], [-1]):
        with pytest.raises(IndexError):
            gm.remove_nodes(g, bad)
    with pytest.raises(ValueError, match="outside"):
        gm.remove_nodes(g, 1.5)
    with pytest.raises(TypeError, match="integers"):
        gm.remove_nodes(g, [1.5, 2.0])
    _derived_equals_built(gm, g, lambda: gm.remove_nodes(g, nodes))
    _derived_equals_built(gm, g, lambda: gm.remove_nodes(g, p, seed=seed))


@pytest.mark.gpu
def test_python_add_edges_and_add_nodes(gm, batch3):
    import torch
    g, h = batch3
    sn, tn, wn = [28, 1, 5], [1, 28, 5], [5.0, 6.0, 7.0]
    s2, t2, w2, n2 = R.add_edges(h["s"], h["t"], h["w"], h["n"], sn, tn, wn)
    new_e = torch.ones((3, 3), device="cuda")
    g2, ed2 = gm.add_edges(g, sn, tn, w=wn, edata=h["edata"], new_edata={"e": new_e})
    _is_graph(g2, s2, t2, w2, n2)
    assert torch.equal(ed2["e"], torch.cat([h["edata"]["e"], new_e])) and torch.equal(g2.x, g.x)
    assert torch.equal(g2.graph_indicator, g.graph_indicator) and g2.num_graphs == 3
    for form in ((sn, tn), (sn, tn, wn)):                                  # the tuple forms
        _is_graph(gm.add_edges(g, form, w=wn), s2, t2, w2, n2)
    _is_graph(gm.add_edges(g, sn, tn), *R.add_edges(h["s"], h["t"], h["w"], h["n"], sn, tn, None))      # missing new weights: ones
    bare = gm.GNNGraph(g.s, g.t, num_nodes=g.num_nodes)
    _is_graph(gm.add_edges(bare, (sn, tn, wn)), *R.add_edges(h["s"], h["t"], None, h["n"], sn, tn, wn))  # missing old weights: ones
    assert gm.add_edges(bare, sn, tn).w is None
    assert gm.add_edges(g, [], []) is g                                    # m == 0: g itself
    grown = gm.add_edges(bare, [30, 2], [1, 33])                           # an index above num_nodes adds nodes
    _is_graph(grown, *R.add_edges(h["s"], h["t"], None, h["n"], [30, 2], [1, 33]))
    assert grown.num_nodes == 33 and gm.add_edges(bare, [30, 2], [1, 33], num_nodes=40).num_nodes == 40
    empty = gm.GNNGraph(torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64), num_nodes=0)
    _is_graph(gm.add_edges(empty, ([1, 3], [2, 1])), np.array([1, 3]), np.array([2, 1]), None, 3)      # transform.jl:160-167
    with pytest.raises(ValueError, match="without node features"):
        gm.add_edges(g, [30], [1])
    with pytest.raises(AssertionError):
        gm.add_edges(g, [0], [1])
    with pytest.raises(ValueError, match="go together"):
        gm.add_edges(g, sn, tn, edata=h["edata"])
    _derived_equals_built(gm, g, lambda: gm.add_edges(g, sn, tn, w=wn))
    # add_nodes
    xn = torch.ones((5, 5), device="cuda")
    g3 = gm.add_nodes(g, 5, x=xn, graph_indicator=[3, 3, 3, 1, 2])
    _is_graph(g3, h["s"], h["t"], h["w"], R.add_nodes(h["n"], 5))
    assert torch.equal(g3.x[:28], g.x) and torch.all(g3.x[28:] == 1) and g3.num_graphs == 3
    assert _np(g3.graph_indicator).tolist() == h["gi"].tolist() + [3, 3, 3, 1, 2]
    assert gm.add_nodes(g, 0) is g and gm.add_nodes(bare, 4).num_nodes == 32 and gm.add_nodes(bare, 4).x is None
    with pytest.raises(ValueError, match="node features"):
        gm.add_nodes(g, 5)
    with pytest.raises(ValueError, match="node features"):
        gm.add_nodes(bare, 5, x=xn)
    with pytest.raises(ValueError, match="graph_indicator"):
        gm.add_nodes(g, 5, x=xn)
    with pytest.raises(ValueError, match="shape"):
        gm.add_nodes(g, 4, x=xn, graph_indicator=[1, 1, 1, 1])
    _derived_equals_built(gm, g, lambda: gm.add_nodes(g, 5, x=xn, graph_indicator=[3, 3, 3, 1, 2]))


@pytest.mark.gpu
def test_python_perturb_edges(gm, batch3):
    import torch
    g, h = batch3
    seed = 77
    s2, t2, w2, n2 = R.perturb_edges(h["s"], h["t"], h["w"], h["n"], 0.5, seed)
    g2 = gm.perturb_edges(g, 0.5, seed=seed)
    _is_graph(g2, s2, t2, w2, n2)
    assert g2.num_edges == 45 + 23 and np.all(w2[45:] == 1.0) and torch.equal(g2.x, g.x)
    assert torch.equal(gm.perturb_edges(g, 0.5, seed=seed).s, g2.s)
    assert not torch.equal(gm.perturb_edges(g, 0.5, seed=seed + 1).s, g2.s)
    assert gm.perturb_edges(g, 0.0) is g
    ring = gm.GNNGraph([1, 2, 3, 4, 5], [2, 3, 4, 5, 1])
    assert gm.perturb_edges(ring, 0.5).num_edges == 8 and gm.perturb_edges(ring, 0.5).w is None       # transform.jl:187-193
    with pytest.raises(AssertionError, match="perturb_ratio must be between 0 and 1"):
        gm.perturb_edges(g, 1.5)
    with pytest.raises(AssertionError, match="at least 2 nodes"):
        gm.perturb_edges(gm.GNNGraph([1], [1]), 1.0)
    _derived_equals_built(gm, g, lambda: gm.perturb_edges(g, 0.5, seed=seed))


@pytest.mark.gpu
def test_other_containers_are_refused_by_name(gm):
    import torch
    sp = gm.GNNGraph.from_sparse(colptr=torch.tensor([1, 2, 3, 3]), rowval=torch.tensor([2, 1]))
    for fn, args in ((gm.remove_nodes, ([1],)), (gm.add_edges, ([1], [2])), (gm.add_nodes, (1,)), (gm.perturb_edges, (0.5,))):
        with pytest.raises(TypeError, match="sparse-matrix graphs"):
            fn(sp, *args)
        with pytest.raises(TypeError, match="expected a GNNGraph"):
            fn(object(), *args)

        class Hetero:
            is_hetero = True
        with pytest.raises(TypeError, match="GNNHeteroGraph is not supported"):
            fn(Hetero(), *args)
        tg = object.__new__(gm.TemporalSnapshotsGNNGraph)
        with pytest.raises(TypeError, match="TemporalSnapshotsGNNGraph is not supported"):
            fn(tg, *args)
