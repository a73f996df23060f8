"""edge_conv_ad: EdgeConv with a one-layer nn, trained on the fused pair-message row kernels (csrc/edge_conv.hip; include/gnnmp.h states the
arithmetic).

Without a GPU: the two exports exist in header, SYMBOLS and library and take const host records; every refusal of the header comes before
any HIP call; the float64 gradient reference (tests/edge_conv_ref.py) agrees with central finite differences and hands Δ to every
maximiser of a tie; the Gaussian cases of the GPU tests keep float32 away from relu's kink and from a change of winner.

On the GPU: integer-valued operands give the bits of the oracle (forward) and of the reference (dP) at every vector width, tail and tile
count, on a multigraph with self loops, duplicate edges, empty rows and a hub destination and source three times the plan's long-row
threshold; Gaussian inputs on device-built kNN graphs stay within 1e-5 of the float64 reference; every output element is written and
nothing else (the slab of tests/abi_cases.py), at any pointer alignment, on a side stream; forward + backward can be recorded into a HIP
graph and replayed; two calls give equal bits; a small DGCNN step has the reference's gradients."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_cases as A  # noqa: E402
import edge_conv_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FWD, GRAD = "gnnmp_edge_conv_f32", "gnnmp_edge_conv_grad_f32"
gpu = pytest.mark.gpu
f32, f64 = np.float32, np.float64
U = 2.0 ** -24
MARGIN = 20         # every discontinuity is at least this many times farther away than float32 is from float64


# ------------------------------------------------------------------------------------------------------------------------------------
# CPU: the ABI
# ------------------------------------------------------------------------------------------------------------------------------------
def test_header_symbols_and_library_carry_the_exports():
    import gnnmp
    from gnnmp import _lib
    header = open(os.path.join(ROOT, "include", "gnnmp.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    internal = header.index("GNNMP_INTERNAL")
    for name in (FWD, GRAD):
        assert f"int {name}(" in header and header.index(f"int {name}(") < internal
        assert name in _lib.SYMBOLS
        assert name in exported
    assert "} gnnmp_edge_conv_t;" in header and "} gnnmp_edge_conv_grad_t;" in header
    assert "GNNlib/src/layers/conv.jl:237-246" in header[:internal]
    assert "tests/test_edge_conv_ad.py" in header[:header.index("#ifndef GNNMP_H")]          # the Conventions paragraph: what is tested
    assert callable(gnnmp.edge_conv_ad)


def test_the_exports_take_const_host_records():
    """device pointers travel in const host records: the table of tests/abi_cases.py owes no case, this file carries the memory-contract
    and capture checks itself"""
    from gnnmp import _lib
    decls, _ = A.parse_header()
    need = A.must_be_covered(decls, _lib.SYMBOLS)
    assert FWD not in need and GRAD not in need
    assert [p[0] for p in decls[FWD]] == ["plan", "job", "C", "stream"]
    assert [p[0] for p in decls[GRAD]] == ["plan", "plan_t", "job", "C", "stream"]
    for name in (FWD, GRAD):
        for pname, is_ptr, is_const, _ in decls[name]:
            assert is_const or not is_ptr, (name, pname)                                        # plans and jobs are const
    assert ctypes.sizeof(_lib.EdgeConvJob) == 24 and ctypes.sizeof(_lib.EdgeConvGradJob) == 40
    assert [getattr(_lib.EdgeConvJob, f).offset for f in ("p", "y", "aggr", "act")] == [0, 8, 16, 20]
    assert [getattr(_lib.EdgeConvGradJob, f).offset for f in ("p", "y", "dy", "dp", "aggr", "act")] == [0, 8, 16, 24, 32, 36]


P = lambda v: ctypes.c_void_p(0x1000 * v) if v else None      # never dereferenced: the call must refuse first  # noqa: E731


class _FakePlan(ctypes.Structure):
    """the head of csrc/common.h's gnnmp_graph {int64 n_src, n_dst, n_edges, n_total; ...}: all the refusals read of a plan"""
    _fields_ = [("n_src", ctypes.c_int64), ("n_dst", ctypes.c_int64), ("n_edges", ctypes.c_int64), ("n_total", ctypes.c_int64),
                ("tail", ctypes.c_char * 1024)]


def _fwd(lib, plan, job=True, p=1, y=2, aggr=0, act=0, C=4):
    from gnnmp import _lib
    j = _lib.EdgeConvJob(P(p), P(y), aggr, act)
    return lib.gnnmp_edge_conv_f32(plan, ctypes.byref(j) if job else None, C, None)


def _grad(lib, plan, plan_t, job=True, p=1, y=2, dy=3, dp=4, aggr=0, act=0, C=4):
    from gnnmp import _lib
    j = _lib.EdgeConvGradJob(P(p), P(y), P(dy), P(dp), aggr, act)
    return lib.gnnmp_edge_conv_grad_f32(plan, plan_t, ctypes.byref(j) if job else None, C, None)


def test_argument_validation_needs_no_gpu():
    """every refusal of the header comes before the first HIP call: on a machine without a device, on pointers that are not memory"""
    from gnnmp import _lib
    lib = _lib.load()
    EINVAL, err = _lib.EINVAL, lib.gnnmp_last_error
    sq, sq_t = _FakePlan(n_src=5, n_dst=5, n_edges=7, n_total=7), _FakePlan(n_src=5, n_dst=5, n_edges=7, n_total=7)
    pl, pt = ctypes.addressof(sq), ctypes.addressof(sq_t)
    for call in (lambda **kw: _fwd(lib, pl, **kw), lambda **kw: _grad(lib, pl, pt, **kw)):
        assert call(job=False) == EINVAL and b"null job" in err()
        assert call(p=None) == EINVAL and b"null p" in err()
        assert call(y=None) == EINVAL and b"null y" in err()
        for C in (0, -3, (1 << 20) + 1, 2 ** 40):
            assert call(C=C) == EINVAL and b"bad C" in err(), C
        for aggr in (-1, 4, 17):
            assert call(aggr=aggr) == EINVAL and b"bad aggr" in err(), aggr
        for act in (-1, 2, 3, 4):                                # softplus, tanh, swish: not covered
            assert call(act=act) == EINVAL and b"bad act" in err(), act
    assert _fwd(lib, None) == EINVAL and b"null plan" in err()
    assert _grad(lib, None, pt) == EINVAL and b"null plan" in err()
    assert _grad(lib, pl, None) == EINVAL and b"null plan_t" in err()
    assert _grad(lib, pl, pt, dy=None) == EINVAL and b"null dy" in err()
    assert _grad(lib, pl, pt, dp=None) == EINVAL and b"null dp" in err()
    # a plan that is not square; a transposed plan of another height, of another edge count
    rect = _FakePlan(n_src=9, n_dst=5, n_edges=7, n_total=7)
    assert _fwd(lib, ctypes.addressof(rect)) == EINVAL and b"not square" in err()
    assert _grad(lib, ctypes.addressof(rect), pt) == EINVAL and b"not square" in err()
    tall = _FakePlan(n_src=6, n_dst=6, n_edges=7, n_total=7)
    assert _grad(lib, pl, ctypes.addressof(tall)) == EINVAL and b"the transposed plan has 6 rows, the plan 5" in err()
    more = _FakePlan(n_src=5, n_dst=5, n_edges=8, n_total=8)
    assert _grad(lib, pl, ctypes.addressof(more)) == EINVAL and b"the transposed plan has 8 edges, the plan 7" in err()
    # N = 0 launches nothing: accepted on a machine without a device
    none = _FakePlan(n_src=0, n_dst=0, n_edges=0, n_total=0)
    assert _fwd(lib, ctypes.addressof(none)) == _lib.OK
    assert _grad(lib, ctypes.addressof(none), ctypes.addressof(none)) == _lib.OK


# ------------------------------------------------------------------------------------------------------------------------------------
# CPU: the references
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("aggr", ["+", "mean"])
def test_reference_gradient_agrees_with_finite_differences(aggr):
    """identity, + and mean are smooth: central differences of the float64 composition, 30 nodes / 200 edges"""
    rng = np.random.default_rng(3)
    n, E, D, C, h = 30, 200, 4, 5, 1e-6
    s, t = rng.integers(0, n, E), rng.integers(0, n, E)
    x, W, b = rng.uniform(-1, 1, (n, D)), rng.uniform(-1, 1, (C, 2 * D)), rng.uniform(-1, 1, C)
    dy = rng.uniform(-1, 1, (n, C))
    ref = R.grad64(s, t, n, x, W, b, aggr, None, dy)
    loss = lambda: float((R.compose(s, t, n, x, W, b, aggr, None)[3] * dy).sum())      # noqa: E731
    for arr, g, what in ((x, ref["dx"], "dx"), (W, ref["dW"], "dW"), (b, ref["db"], "db")):
        fd = np.zeros_like(arr)
        for i in np.ndindex(arr.shape):
            keep = arr[i]
            arr[i] = keep + h
            hi = loss()
            arr[i] = keep - h
            lo = loss()
            arr[i] = keep
            fd[i] = (hi - lo) / (2 * h)
        assert np.abs(fd - g).max() <= 1e-6 * max(np.abs(g).max(), 1.0), (what, np.abs(fd - g).max())


def test_every_maximiser_of_a_tie_receives_delta():
    """a hand-made 4-node graph: nodes 1 and 2 carry the same features, both point at node 0 (and so does node 3, lower) — the two
    messages tie exactly at the maximum and BOTH receive Δ, in the composition's pullback and in the split formulation's dP"""
    s, t, n = np.array([1, 2, 3]), np.array([0, 0, 0]), 4
    x = np.array([[0.0, 0.0], [1.0, 2.0], [1.0, 2.0], [-1.0, -1.0]])
    W = np.array([[1.0, 0.0, 1.0, 1.0]])                         # C = 1: pre = x_i[0] + (x_j - x_i)[0] + (x_j - x_i)[1]
    dy = np.array([[5.0], [0.0], [0.0], [0.0]])
    ref = R.grad64(s, t, n, x, W, None, "max", None, dy)
    assert np.array_equal(ref["pre"][:, 0], [3.0, 3.0, -2.0]) and ref["y"][0, 0] == 3.0
    assert np.array_equal(ref["g"][:, 0], [5.0, 5.0, 0.0])        # not 2.5 / 2.5 (torch.amax), not one winner
    assert np.array_equal(ref["dx"][1], ref["dx"][2]) and np.array_equal(ref["dx"][1], [5.0, 5.0]) and not ref["dx"][3].any()
    P32 = R.stack_p(x, W, None, f32)
    y32 = R.fused(s, t, n, P32, 1, "max", None)[0]
    dP = R.grad_p(s, t, n, P32, 1, y32, dy.astype(f32), "max", None)
    assert np.array_equal(dP[:, 0], [10.0, 0.0, 0.0, 0.0])        # dA_0 = both Δ
    assert np.array_equal(dP[:, 1], [-10.0, 5.0, 5.0, 0.0])       # dB_j - dA_j
    # relu's exact 0: every message of node 3's row below is <= 0, the extremum is relu's 0, every edge "wins" and relu' stops them all
    s2, t2 = np.array([0, 0]), np.array([3, 3])
    ref = R.grad64(s2, t2, n, x, -np.abs(W), None, "max", "relu", np.array([[0.0], [0.0], [0.0], [7.0]]))
    assert ref["y"][3, 0] == 0.0 and not ref["g"].any()


def _assert_conditioned(what, cond):
    dev, kink, gap = cond
    assert dev < 1e-4, (what, dev)
    assert kink >= MARGIN * dev, f"{what}: the smallest |pre| {kink:.2e} is within {MARGIN} x {dev:.2e} of relu's kink"
    assert gap >= MARGIN * dev, f"{what}: the smallest top-two gap {gap:.2e} is within {MARGIN} x {dev:.2e} of a change of winner"


@pytest.mark.parametrize("name", sorted(R.GAUSSIAN))
def test_the_gaussian_cases_are_well_conditioned(name):
    """THE CONDITION ON THE INPUTS: max / min winners and relu's kink are discontinuities; the inputs keep float32 away from them (the
    graph here is the float64 brute-force kNN graph; the GPU tests assert the same on the graph the device built)"""
    x, gi, k, W, b, _ = R.gaussian_case(name)
    s, t = R.knn_cpu(x, k, gi)
    _assert_conditioned(name, R.conditioning(s, t, len(x), x, W, b))


def test_the_dgcnn_case_is_well_conditioned():
    x, gi, k, Ws, bs, _ = R.dgcnn_case()
    n = len(x)
    s1, t1 = R.knn_cpu(x, k, gi)
    _assert_conditioned("layer 1", R.conditioning(s1, t1, n, x, Ws[0], bs[0]))
    h1 = R.compose(s1, t1, n, x, Ws[0], bs[0], "max", "relu")[3].astype(f32)
    s2, t2 = R.knn_cpu(h1, k, gi)
    _assert_conditioned("layer 2", R.conditioning(s2, t2, n, h1, Ws[1], bs[1]))


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU helpers
# ------------------------------------------------------------------------------------------------------------------------------------
def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def close(got, ref, what, tol=1e-5):
    got, ref = np.asarray(got, f64), np.asarray(ref, f64)
    assert got.shape == ref.shape, what
    assert np.all(np.isfinite(got)), f"{what}: non-finite"
    err, scale = np.linalg.norm(got - ref), np.linalg.norm(ref)
    print(f"{what}: |got - ref| = {err:.3e}, |ref| = {scale:.3e}")
    assert err <= tol * scale, f"{what}: {err:.3e} > {tol:g} * {scale:.3e}"


def layer(W, b, sigma, aggr):
    import gnnmp
    C, D2 = W.shape
    nn = gnnmp.Dense((D2, C), sigma)
    nn.weight, nn.bias = dev(W.astype(f32)), (None if b is None else dev(b.astype(f32)))
    return gnnmp.EdgeConv(nn, aggr=aggr)


def layer_grads(l, g, x, dy):
    """(y, dx, dW, db) of edge_conv_ad as numpy arrays"""
    import torch
    import gnnmp
    xt = dev(x.astype(f32)).requires_grad_(True)
    l.nn.weight.requires_grad_(True)
    l.nn.bias.requires_grad_(True)
    for p in (l.nn.weight, l.nn.bias):
        p.grad = None
    y = gnnmp.edge_conv_ad(l, g, xt)
    y.backward(dev(dy.astype(f32)))
    torch.cuda.synchronize()
    return tuple(v.detach().cpu().numpy() for v in (y, xt.grad, l.nn.weight.grad, l.nn.bias.grad))


def call_fwd(lib, plan, p, y, aggr, act, C, stream=None):
    from gnnmp import _lib
    job = _lib.EdgeConvJob(p, y, aggr, act)
    return lib.gnnmp_edge_conv_f32(plan, ctypes.byref(job), C, stream)


def call_grad(lib, plan, plan_t, p, y, dy, dp, aggr, act, C, stream=None):
    from gnnmp import _lib
    job = _lib.EdgeConvGradJob(p, y, dy, dp, aggr, act)
    return lib.gnnmp_edge_conv_grad_f32(plan, plan_t, ctypes.byref(job), C, stream)


@pytest.fixture(scope="module")
def lib():
    import torch
    assert torch.cuda.is_available()
    from gnnmp import _lib
    return _lib.load()


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU 1: exact
# ------------------------------------------------------------------------------------------------------------------------------------
N_EXACT = 300


def exact_edges(thr):
    """a random multigraph on 300 nodes, about 2400 edges: self loops, duplicate edges, rows with no in-edges (nodes 0, 150, 299), rows with
    no out-edges (nodes 1, 151, 298), destination 7 and source 9 of degree 3 thr + 7 (three times the plan's long-row threshold)"""
    rng = np.random.default_rng(11)
    n, hub = N_EXACT, 3 * thr + 7
    no_in, no_out = np.array([0, 150, 299]), np.array([1, 151, 298])
    srcs, dsts = np.setdiff1d(np.arange(n), no_out), np.setdiff1d(np.arange(n), no_in)
    s, t = rng.choice(srcs, 2000), rng.choice(dsts, 2000)
    s[:12] = t[:12]                                              # self loops (nodes that may be both)
    ok = ~np.isin(s[:12], no_out)
    s[:12][~ok] = 5
    t[:12][~ok] = 5
    s[12:40], t[12:40] = s[40:68], t[40:68]                      # duplicate edges
    s = np.concatenate([s, rng.choice(srcs, hub), np.full(hub, 9)])
    t = np.concatenate([t, np.full(hub, 7), rng.choice(dsts, hub)])
    perm = rng.permutation(len(s))
    return s[perm].astype(np.int64), t[perm].astype(np.int64), hub


@pytest.fixture(scope="module")
def exact_graph(lib):
    import gnnmp
    thr = A.plan_threshold(lib, 2400)
    s, t, hub = exact_edges(thr)
    n = N_EXACT
    g = gnnmp.GNNGraph(dev(s + 1), dev(t + 1), num_nodes=n)
    plan, plan_t = g.plan(False), g.plan_transposed(False)
    assert plan.long_thresh == thr == plan_t.long_thresh and plan.n_long >= 1 and plan_t.n_long >= 1      # the plans DO split the hubs
    indeg, outdeg = np.bincount(t, minlength=n), np.bincount(s, minlength=n)
    assert indeg[7] >= hub and outdeg[9] >= hub and (indeg == 0).sum() >= 3 and (outdeg == 0).sum() >= 3
    assert (s == t).sum() >= 12 and len(s) - len(set(zip(s.tolist(), t.tolist()))) >= 28
    assert len(s) >= 2300
    return g, s, t


def exact_operands(C):
    rng = np.random.default_rng(100 + C)
    D = 5
    x = rng.integers(-3, 4, (N_EXACT, D)).astype(f32)
    W = rng.integers(-2, 3, (C, 2 * D)).astype(f32)
    b = rng.integers(-3, 4, C).astype(f32)
    dy = rng.integers(-2, 3, (N_EXACT, C)).astype(f32)
    return x, W, b, dy


@gpu
@pytest.mark.parametrize("sigma", R.ACTS, ids=["identity", "relu"])
@pytest.mark.parametrize("aggr", R.AGGRS)
@pytest.mark.parametrize("C", [1, 3, 8, 64, 260])
def test_exact_on_integer_operands(lib, exact_graph, C, aggr, sigma):
    """integer-valued operands, everything below 2^24: y has the bits of the oracle, dP the bits of the reference (mean: of the reference
    evaluated in float32 in edge order); the layer's dx, dW, db are within 1e-5"""
    import torch
    from oracle import more_layers as ML
    g, s, t = exact_graph
    n = N_EXACT
    x, W, b, dy = exact_operands(C)
    Pm = R.stack_p(x, W, b, f32)
    assert np.array_equal(Pm.astype(f64), R.stack_p(x, W, b, f64)) and np.abs(Pm).max() * (np.bincount(t).max() + 2) < 2 ** 24
    Pd, dyd = dev(Pm), dev(dy)
    yd = torch.full((n, C), float("nan"), dtype=torch.float32, device="cuda")
    dPd = torch.full((n, 2 * C), float("nan"), dtype=torch.float32, device="cuda")
    ac, sc = R.AGGR_CODE[aggr], R.ACT_CODE[sigma]
    plan, plan_t = g.plan(False).handle, g.plan_transposed(False).handle
    ptr = lambda v: ctypes.c_void_p(v.data_ptr())      # noqa: E731
    assert call_fwd(lib, plan, ptr(Pd), ptr(yd), ac, sc, C) == A.OK, lib.gnnmp_last_error()
    assert call_grad(lib, plan, plan_t, ptr(Pd), ptr(yd), ptr(dyd), ptr(dPd), ac, sc, C) == A.OK, lib.gnnmp_last_error()
    torch.cuda.synchronize()
    y, dP = yd.cpu().numpy(), dPd.cpu().numpy()
    y_ref = ML.edge_conv(s + 1, t + 1, n, x, [(W, b, sigma)], aggr)
    assert np.array_equal(bits(y), bits(y_ref)), f"y: {(bits(y) != bits(y_ref)).sum()} elements differ from the oracle's bits"
    ref = R.grad64(s, t, n, x, W, b, aggr, sigma, dy)
    if aggr == "mean":
        dP_ref = R.grad_p(s, t, n, Pm, C, y_ref, dy, aggr, sigma)
        assert dP_ref.dtype == f32
    else:
        dP_ref = R.dp_from_g(s, t, n, ref["g"])
        assert np.array_equal(dP_ref, dP_ref.astype(f32).astype(f64))        # exact in float32
    assert np.array_equal(bits(dP), bits(dP_ref)), f"dP: {(bits(dP) != bits(dP_ref)).sum()} elements differ from the reference's bits"
    # the layer: the same numbers through dense, the two exports and the dense adjoints
    yl, dx, dW, db = layer_grads(layer(W, b, sigma, aggr), g, x, dy)
    empty = ~np.isfinite(y_ref)                                   # rows without in-edges under max / min: the identity, -Inf / +Inf
    assert np.array_equal(yl[empty], y_ref[empty])
    close(yl[~empty], y_ref[~empty], "y of the layer")
    close(dx, ref["dx"], "dx")
    close(dW, ref["dW"], "dW")
    close(db, ref["db"], "db")


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU 2: Gaussian inputs on the device's own kNN graphs
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gaussian_graphs():
    """per case: the graph gnnmp.knn_graph builds (with graph_indicator), its 0-based edges, and the conditioning of the case ON that graph"""
    import gnnmp
    out = {}
    for name in R.GAUSSIAN:
        x, gi, k, W, b, _ = R.gaussian_case(name)
        g = gnnmp.knn_graph(dev(x), k, graph_indicator=dev(gi + 1))
        s, t = g.s.cpu().numpy() - 1, g.t.cpu().numpy() - 1
        assert len(s) == k * len(x) and np.array_equal(gi[s], gi[t])
        out[name] = (g, s, t, R.conditioning(s, t, len(x), x, W, b))
    return out


def forward_bound(s, t, n, x, W, b, aggr, sigma):
    """element-wise bound on |y - y_float64| in the form of tests/test_dense_fallbacks.py: (operations) * 2^-24 * (sum of magnitudes).
    Per edge pre_e = P[i][c] - P[i][C+c] + P[j][C+c]: each entry of P is a dense output — the dense core's bound relative to
    sum |w||x| (+ |b|) is max(SPLIT_BOUND, (D + 2) * 2^-24) — and the two additions round twice more on the same magnitude.  relu is
    1-Lipschitz; + adds deg roundings on sum |m|, mean one more for the division; max / min move by at most the largest perturbation of
    a candidate."""
    D = x.shape[1]
    xa, Wa = np.abs(x.astype(f64)), np.abs(W.astype(f64))
    mag_i = xa @ Wa[:, :D].T + np.abs(b.astype(f64)) + xa @ Wa[:, D:].T            # |P[i][c]| + |P[i][C+c]| majorants
    mag_e = mag_i[t] + (xa @ Wa[:, D:].T)[s]
    e_pre = (max(A.SPLIT_BOUND, (D + 2) * U) + 3 * U) * mag_e
    m = np.abs(R.compose(s, t, n, x, W, b, aggr, sigma)[2])
    deg = np.bincount(t, minlength=n)[:, None].astype(f64)
    if aggr in ("+", "mean"):
        bound = R.fold(t, n, e_pre, "+") + (deg + 1) * U * (R.fold(t, n, m, "+") + R.fold(t, n, e_pre, "+"))
        return bound / np.maximum(deg, 1) if aggr == "mean" else bound
    return R.fold(t, n, e_pre, "max")


@gpu
@pytest.mark.parametrize("sigma", R.ACTS, ids=["identity", "relu"])
@pytest.mark.parametrize("aggr", R.AGGRS)
@pytest.mark.parametrize("name", sorted(R.GAUSSIAN))
def test_gaussian_inputs_on_device_knn_graphs(gaussian_graphs, name, aggr, sigma):
    from oracle import more_layers as ML
    g, s, t, cond = gaussian_graphs[name]
    _assert_conditioned(f"{name} on the device's graph", cond)
    x, _, _, W, b, dy = R.gaussian_case(name)
    n = len(x)
    y, dx, dW, db = layer_grads(layer(W, b, sigma, aggr), g, x, dy)
    close(y, ML.edge_conv(s + 1, t + 1, n, x, [(W, b, sigma)], aggr).astype(f64), "y against the oracle")
    ref = R.grad64(s, t, n, x, W, b, aggr, sigma, dy)
    worst = float((np.abs(y.astype(f64) - ref["y"]) / forward_bound(s, t, n, x, W, b, aggr, sigma)).max())
    print(f"y element-wise: {worst:.3f} of the fp32 summation bound")
    assert worst <= 1.0, f"y: element-wise error is {worst:.2f} x the fp32 summation bound"
    close(dx, ref["dx"], "dx")
    close(dW, ref["dW"], "dW")
    close(db, ref["db"], "db")


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU 3: the memory contract
# ------------------------------------------------------------------------------------------------------------------------------------
CONTRACT_GRAPH = A.random_graph("edge_conv", 40, 100, 21)
assert (CONTRACT_GRAPH.indeg() == 0).any() and (np.bincount(CONTRACT_GRAPH.s - 1, minlength=40) == 0).any()      # rows without edges


def contract_case(C, aggr, sigma, seed=0):
    """integer operands on a small random multigraph with rows without in-edges and rows without out-edges: (graph, P, y, Δ, dP)"""
    g = CONTRACT_GRAPH
    s, t, n = g.s - 1, g.t - 1, g.n
    rng = np.random.default_rng(50 + C + seed)
    x, W = rng.integers(-3, 4, (n, 5)).astype(f32), rng.integers(-2, 3, (C, 10)).astype(f32)
    b, dy = rng.integers(-3, 4, C).astype(f32), rng.integers(-2, 3, (n, C)).astype(f32)
    Pm = R.stack_p(x, W, b, f32)
    y = R.fused(s, t, n, Pm, C, aggr, sigma)[0]
    dP = R.grad_p(s, t, n, Pm, C, y, dy, aggr, sigma)
    return g, Pm, y, dy, dP


@gpu
@pytest.mark.parametrize("C", [8, 6])
def test_memory_contract(lib, C):
    """every element of y and dP written, no store before or after an array or into p / y / dy, with each array in turn shifted to 16-,
    8- and 4-byte alignment (C = 8: 16-byte lanes narrow to 8 and 4; C = 6: 8-byte lanes narrow to 4), on a side stream"""
    import torch
    side = torch.cuda.Stream()
    sp = ctypes.c_void_p(side.cuda_stream)
    plans = A.Plans(lib)
    try:
        k = 0
        for export, names in ((FWD, ("p", "y")), (GRAD, ("p", "y", "dy", "dp"))):
            for shifts in [{}] + [{nm: A.SHIFTS[a]} for nm in names for a in ("a16", "a8", "a4")]:
                aggr, sigma = R.AGGRS[k % 4], R.ACTS[(k // 4) % 2]
                k += 1
                g, Pm, y, dy, dP = contract_case(C, aggr, sigma)
                plan, plan_t = plans.get(A.Pl(g)), plans.get(A.Pl(g, T=True))
                ac, sc = R.AGGR_CODE[aggr], R.ACT_CODE[sigma]
                if export == FWD:
                    slab = A.Slab([A.Arr("p", "in", Pm), A.Arr("y", "out", shape=y.shape)], "cuda", shifts)
                    torch.cuda.synchronize()
                    rc = call_fwd(lib, plan, slab.ptr("p"), slab.ptr("y"), ac, sc, C, sp)
                    want = {"y": A.E(y, tol="exact")}
                else:
                    slab = A.Slab([A.Arr("p", "in", Pm), A.Arr("y", "in", y), A.Arr("dy", "in", dy), A.Arr("dp", "out", shape=dP.shape)],
                                  "cuda", shifts)
                    torch.cuda.synchronize()
                    rc = call_grad(lib, plan, plan_t, slab.ptr("p"), slab.ptr("y"), slab.ptr("dy"), slab.ptr("dp"), ac, sc, C, sp)
                    want = {"dp": A.E(dP, tol="exact")}
                torch.cuda.synchronize()
                assert rc == A.OK, (export, shifts, lib.gnnmp_last_error())
                problems = slab.check(want)
                assert not problems, (export, aggr, sigma, shifts, problems)
        assert k == 7 + 13
    finally:
        plans.close()


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU 4 and 5: capture, determinism
# ------------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("aggr,sigma", [("max", "relu"), ("mean", None)])
def test_forward_and_backward_record_into_a_hip_graph(lib, aggr, sigma):
    """one eager call; forward + backward recorded (capture_error_mode = thread_local: a host wait or an allocation would be an error);
    the outputs still hold poison after the capture; the replay has the eager bits; new inputs at the same addresses give the new
    reference; two replays back to back give those bits again"""
    import torch
    C = 8
    g, Pm, y, dy, dP = contract_case(C, aggr, sigma)
    _, Pm2, y2, dy2, dP2 = contract_case(C, aggr, sigma, seed=1)
    assert not np.array_equal(Pm, Pm2) and not np.array_equal(dP, dP2)
    ac, sc = R.AGGR_CODE[aggr], R.ACT_CODE[sigma]
    side = torch.cuda.Stream()
    sp = ctypes.c_void_p(side.cuda_stream)
    plans = A.Plans(lib)
    try:
        plan, plan_t = plans.get(A.Pl(g)), plans.get(A.Pl(g, T=True))
        slab = A.Slab([A.Arr("p", "in", Pm), A.Arr("dy", "in", dy), A.Arr("y", "out", shape=y.shape), A.Arr("dp", "out", shape=dP.shape)])

        def both():
            rc = call_fwd(lib, plan, slab.ptr("p"), slab.ptr("y"), ac, sc, C, sp)
            return rc or call_grad(lib, plan, plan_t, slab.ptr("p"), slab.ptr("y"), slab.ptr("dy"), slab.ptr("dp"), ac, sc, C, sp)

        want = {"y": A.E(y, tol="exact"), "dp": A.E(dP, tol="exact")}
        torch.cuda.synchronize()
        assert both() == A.OK, lib.gnnmp_last_error()
        torch.cuda.synchronize()
        assert not slab.check(want)
        eager = slab.outputs()
        slab.reload()
        graph = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            graph.capture_begin(capture_error_mode="thread_local")
            try:
                rc = both()
            finally:
                graph.capture_end()
        torch.cuda.synchronize()
        assert rc == A.OK, lib.gnnmp_last_error()
        assert not slab.check({}, untouched=True), "work ran while the calls were being recorded"
        graph.replay()
        torch.cuda.synchronize()
        assert not slab.check(want)
        got = slab.outputs()
        assert all(np.array_equal(got[k], eager[k]) for k in eager)
        slab.reload({"p": Pm2, "dy": dy2})
        graph.replay()
        torch.cuda.synchronize()
        want2 = {"y": A.E(y2, tol="exact"), "dp": A.E(dP2, tol="exact")}
        assert not slab.check(want2)
        second = slab.outputs()
        graph.replay()
        graph.replay()
        torch.cuda.synchronize()
        assert not slab.check(want2)
        got = slab.outputs()
        assert all(np.array_equal(got[k], second[k]) for k in second)
        del graph
    finally:
        plans.close()


@gpu
def test_two_calls_give_equal_bits(gaussian_graphs):
    g, _, _, _ = gaussian_graphs["cond"]
    x, _, _, W, b, dy = R.gaussian_case("cond")
    for aggr, sigma in (("+", "relu"), ("mean", None), ("max", "relu"), ("min", None)):
        l = layer(W, b, sigma, aggr)
        first, again = layer_grads(l, g, x, dy), layer_grads(l, g, x, dy)
        for a, c, what in zip(first, again, ("y", "dx", "dW", "db")):
            assert np.array_equal(bits(a), bits(c)), (aggr, sigma, what)


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU 6: what edge_conv_ad refuses
# ------------------------------------------------------------------------------------------------------------------------------------
@gpu
def test_edge_conv_ad_refuses_by_name(gaussian_graphs):
    import torch
    import gnnmp
    g, _, _, _ = gaussian_graphs["cond"]
    x, _, _, W, b, _ = R.gaussian_case("cond")
    xt = dev(x)
    two = gnnmp.EdgeConv([gnnmp.Dense((10, 12), "relu"), gnnmp.Dense((12, 12))], aggr="max")
    with pytest.raises(NotImplementedError, match="one-layer nn"):
        gnnmp.edge_conv_ad(two, g, xt)
    for sigma in (torch.tanh, torch.sigmoid):
        with pytest.raises(ValueError, match="identity and relu"):
            gnnmp.edge_conv_ad(layer(W, b, sigma, "max"), g, xt)
    with pytest.raises(ValueError, match="unsupported activation"):
        gnnmp.edge_conv_ad(layer(W, b, "softplus", "max"), g, xt)
    with pytest.raises(NotImplementedError, match="bipartite"):
        gnnmp.edge_conv_ad(layer(W, b, "relu", "max"), g, (xt, xt))
    with pytest.raises(ValueError, match="aggregation"):
        gnnmp.edge_conv_ad(layer(W, b, "relu", "median"), g, xt)
    # under no_grad it is simply the fused forward, and the composition (the parent's path) agrees with it
    with torch.no_grad():
        l = layer(W, b, "relu", "max")
        y = gnnmp.edge_conv_ad(l, g, xt)
        assert not y.requires_grad
        close(y.cpu().numpy(), gnnmp.edge_conv(l, g, xt).cpu().numpy(), "fused forward against gnnmp.edge_conv")


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU 7: a small DGCNN step
# ------------------------------------------------------------------------------------------------------------------------------------
@gpu
def test_a_small_dgcnn_step():
    """knn_graph(x) -> edge_conv_ad -> knn_graph(h, graph_indicator) -> edge_conv_ad -> global_pool_ad; 4 clouds of 64 points, C = 16 then
    24: the gradients of both layers against the float64 reference evaluated on the edge indices the device produced"""
    import torch
    import gnnmp
    from gnnmp.backward import global_pool_ad
    x, gi, k, Ws, bs, Rm = R.dgcnn_case()
    n = len(x)
    gid = dev(gi + 1)
    ls = [layer(Ws[i], bs[i], "relu", "max") for i in range(2)]
    for l in ls:
        l.nn.weight.requires_grad_(True)
        l.nn.bias.requires_grad_(True)
    xt = dev(x).requires_grad_(True)
    g1 = gnnmp.knn_graph(xt.detach(), k, graph_indicator=gid)
    h1 = gnnmp.edge_conv_ad(ls[0], g1, xt)
    g2 = gnnmp.knn_graph(h1.detach(), k, graph_indicator=gid)
    h2 = gnnmp.edge_conv_ad(ls[1], g2, h1)
    pooled = global_pool_ad(gnnmp.GlobalPool("mean"), g2, h2)
    (pooled * dev(Rm)).sum().backward()
    torch.cuda.synchronize()
    edges = [(g.s.cpu().numpy() - 1, g.t.cpu().numpy() - 1) for g in (g1, g2)]
    h1_ref, h2_ref, grads, dx_ref = R.dgcnn_grad64(edges, gi, x, Ws, bs, Rm)
    _assert_conditioned("layer 1", R.conditioning(*edges[0], n, x, Ws[0], bs[0]))
    _assert_conditioned("layer 2", R.conditioning(*edges[1], n, h1_ref.astype(f32), Ws[1], bs[1]))
    close(h1.detach().cpu().numpy(), h1_ref, "h1")
    close(h2.detach().cpu().numpy(), h2_ref, "h2")
    for i, (l, (dW, db)) in enumerate(zip(ls, grads)):
        close(l.nn.weight.grad.cpu().numpy(), dW, f"dW of layer {i + 1}")
        close(l.nn.bias.grad.cpu().numpy(), db, f"db of layer {i + 1}")
    close(xt.grad.cpu().numpy(), dx_ref, "dx")
