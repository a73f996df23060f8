"""nn_conv_ad: NNConv trained on the one-pass per-edge-matrix adjoint (csrc/nn_grad.hip; include/gnnmp.h states the arithmetic).

Without a GPU: the export exists in header, SYMBOLS and library and takes a const plan and a const host record; every refusal of the header
comes before any HIP call; the float64 gradient reference (tests/nn_conv_ref.py) agrees with central finite differences; the operands of
every GPU case keep the float32 restatement, in the header's summation order, within 2e-6 of float64 and every relu away from the kink.

On the GPU: dx and dwe of the export within 1e-5 of float64 at a single lane, tails in both dimensions, several in-channel tiles, lanes
that own more than one output and the workload's 64 x 64, on a multigraph with self loops, repeated edges, a row without in-edges, a row
without out-edges and a hub destination and source of 600 edges; the layer's y, dx, de, dW, db and nn's gradients within 1e-5 of the
reference's composition, y bit-equal to gnnmp.nn_conv; every output element written and nothing else (the slab of tests/abi_cases.py) at
any pointer alignment; the export recorded into a HIP graph without an eager call first; two calls give equal bits; empty graphs; the
refusals of nn_conv_ad; a small MPNN step on a device-built radius graph."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_cases as A  # noqa: E402
import nn_conv_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRAD = "gnnmp_nn_conv_grad_f32"
gpu = pytest.mark.gpu
f32, f64 = np.float32, np.float64
FIELDS = ("x", "we", "dm", "dx", "dwe")


# ------------------------------------------------------------------------------------------------------------------------------------
# CPU: the ABI
# ------------------------------------------------------------------------------------------------------------------------------------
def test_header_symbols_and_library_carry_the_export():
    import gnnmp
    from gnnmp import _lib
    header = open(os.path.join(ROOT, "include", "gnnmp.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    internal = header.index("GNNMP_INTERNAL")
    assert f"int {GRAD}(" in header and header.index(f"int {GRAD}(") < internal
    assert GRAD in _lib.SYMBOLS and GRAD in exported
    assert "} gnnmp_nn_conv_grad_t;" in header
    assert "GNNlib/src/layers/conv.jl:260-273" in header[header.index("The pullback of NNConv"):internal]
    assert "tests/test_nn_conv_ad.py" in header[:header.index("#ifndef GNNMP_H")]           # the Conventions paragraph: what is tested
    assert callable(gnnmp.nn_conv_ad)


def test_the_export_takes_a_const_plan_and_a_const_host_record():
    """device pointers travel in a const host record: the table of tests/abi_cases.py owes no case, this file carries the memory-contract
    and capture checks itself.  The ctypes record has the layout of the header's struct."""
    from gnnmp import _lib
    decls, _ = A.parse_header()
    assert GRAD not in A.must_be_covered(decls, _lib.SYMBOLS)
    assert [p[0] for p in decls[GRAD]] == ["plan_t", "job", "Din", "Dout", "stream"]
    for pname, is_ptr, is_const, _ in decls[GRAD]:
        assert is_const or not is_ptr, pname
    header = open(os.path.join(ROOT, "include", "gnnmp.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} gnnmp_nn_conv_grad_t;", header).group(1)
    body = re.sub(r"/\*.*?\*/", " ", body, flags=re.S)
    fields, offsets, off = [], [], 0
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        assert "*" in decl, decl                    # pointers only
        for nme in re.sub(r"^(const\s+)?float\s+", "", decl).split(","):
            fields.append(nme.strip().lstrip("*"))
            offsets.append(off)
            off += 8
    assert tuple(fields) == FIELDS == tuple(f for f, _ in _lib.NNConvGradJob._fields_)
    assert [getattr(_lib.NNConvGradJob, f).offset for f in FIELDS] == offsets == [0, 8, 16, 24, 32]
    assert ctypes.sizeof(_lib.NNConvGradJob) == 40


P = lambda v: ctypes.c_void_p(0x1000 * v) if v else None      # never dereferenced: the call must refuse first  # noqa: E731


class _FakePlan(ctypes.Structure):
    """the head of csrc/common.h's gnnmp_graph {int64 n_src, n_dst, n_edges, n_total; ...}: all the refusals read of a plan"""
    _fields_ = [("n_src", ctypes.c_int64), ("n_dst", ctypes.c_int64), ("n_edges", ctypes.c_int64), ("n_total", ctypes.c_int64),
                ("tail", ctypes.c_char * 1024)]


def _grad(lib, plan_t, job=True, x=1, we=2, dm=3, dx=4, dwe=5, Din=4, Dout=4):
    from gnnmp import _lib
    j = _lib.NNConvGradJob(P(x), P(we), P(dm), P(dx), P(dwe))
    return lib.gnnmp_nn_conv_grad_f32(plan_t, ctypes.byref(j) if job else None, Din, Dout, None)


def test_argument_validation_needs_no_gpu():
    """every refusal of the header comes before the first HIP call: on a machine without a device, on pointers that are not memory"""
    from gnnmp import _lib
    lib = _lib.load()
    EINVAL, err = _lib.EINVAL, lib.gnnmp_last_error
    sq = _FakePlan(n_src=5, n_dst=5, n_edges=7, n_total=7)
    pt = ctypes.addressof(sq)
    assert _grad(lib, None) == EINVAL and b"null plan_t" in err()
    assert _grad(lib, pt, job=False) == EINVAL and b"null job" in err()
    assert _grad(lib, pt, x=None) == EINVAL and b"null x" in err()
    assert _grad(lib, pt, dm=None) == EINVAL and b"null dm" in err()
    assert _grad(lib, pt, dx=None, dwe=None) == EINVAL and b"dx and dwe are both null" in err()
    assert _grad(lib, pt, we=None) == EINVAL and b"dx without we" in err()
    for D in (0, -3, (1 << 16) + 1, 2 ** 40):
        assert _grad(lib, pt, Din=D) == EINVAL and b"bad Din" in err(), D
        assert _grad(lib, pt, Dout=D) == EINVAL and b"bad Dout" in err(), D
    rect = _FakePlan(n_src=9, n_dst=5, n_edges=7, n_total=7)
    assert _grad(lib, ctypes.addressof(rect)) == EINVAL and b"not square" in err()
    loops = _FakePlan(n_src=5, n_dst=5, n_edges=7, n_total=12)
    assert _grad(lib, ctypes.addressof(loops)) == EINVAL and b"self loops" in err()
    # N = 0 launches nothing: accepted on a machine without a device — with and without the optional pointers, at the largest sizes
    none = _FakePlan(n_src=0, n_dst=0, n_edges=0, n_total=0)
    assert _grad(lib, ctypes.addressof(none)) == _lib.OK
    assert _grad(lib, ctypes.addressof(none), dwe=None) == _lib.OK
    assert _grad(lib, ctypes.addressof(none), dx=None, we=None, Din=1 << 16, Dout=1 << 16) == _lib.OK


# ------------------------------------------------------------------------------------------------------------------------------------
# CPU: the references
# ------------------------------------------------------------------------------------------------------------------------------------
def _params(x, e, nn, W, b):
    """[(name, array)] of everything the layer is differentiable in"""
    items = [("dx", x), ("de", e), ("dW", W), ("db", b)]
    for i, (Wn, bn, _) in enumerate(nn):
        items += [(f"nn{i}.dW", Wn), (f"nn{i}.db", bn)]
    return items


@pytest.mark.parametrize("depth", [1, 2])
@pytest.mark.parametrize("sigma", [None, "relu"])
@pytest.mark.parametrize("aggr", ["+", "mean"])
def test_reference_gradient_agrees_with_finite_differences(aggr, sigma, depth):
    """central differences of the float64 composition: N = 30, E = 200, ein = 3, in = 4, out = 5, h = 1e-6, for dx, de, dW, db and every
    parameter of nn; every relu pre-activation (the layer's own and nn's hidden layer) is at least 100 h off the kink"""
    h = 1e-6
    s, t, n, x, e, nn, W, b, dy = R.fd_case(depth, sigma)
    ref = R.grad64(s, t, n, x, e, nn, W, b, sigma, aggr, dy)
    assert len(ref["pres"]) == depth - 1
    for pre in ref["pres"] + ([ref["z"]] if sigma == "relu" else []):
        assert np.abs(pre).min() > 100 * h
    loss = lambda: float((R.compose(s, t, n, x, e, nn, W, b, sigma, aggr)[4] * dy).sum())      # noqa: E731
    want = dict(R.flat(ref))
    for what, arr in _params(x, e, nn, W, b):
        g = want[what]
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


def test_the_graph_is_the_multigraph_of_cg_conv_ref():
    s, t = R.graph()
    R.assert_graph(s, t)
    assert len(s) == R.N_EDGES


LAYER_CASES = [(shape, depth, sigma, aggr, bias) for shape in R.LAYER_SHAPES for depth in (1, 2) for sigma, aggr, bias in R.LAYER_VARIANTS]


@pytest.mark.parametrize("Din,Dout", R.KERNEL_SHAPES)
def test_the_kernel_cases_are_well_conditioned(Din, Dout):
    """THE CONDITION ON THE INPUTS, not a measurement: dx and dwe evaluated in float32 by the header's formulas in the header's order are
    within 2e-6, norm-wise, of float64 — a fifth of the 1e-5 bar"""
    s, t = R.graph()
    worst = R.kernel_condition(s, t, R.kernel_case(Din, Dout), Din, Dout)
    assert worst <= R.COND, f"the float32 restatement is {worst:.2e} from float64 (bound {R.COND:g})"


@pytest.mark.parametrize("shape,depth,sigma,aggr,bias", LAYER_CASES)
def test_the_layer_cases_are_well_conditioned(shape, depth, sigma, aggr, bias):
    s, t = R.graph()
    worst, ratio = R.layer_condition(s, t, R.layer_case(shape, depth), sigma, aggr, bias)
    assert worst <= R.COND, f"the float32 restatement is {worst:.2e} from float64 (bound {R.COND:g})"
    assert ratio >= R.MARGIN, f"the smallest relu pre-activation is only {ratio:.1f} x its float32-float64 deviation"


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU helpers
# ------------------------------------------------------------------------------------------------------------------------------------
def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def close(got, ref, what, tol=1e-5):
    """the project's parity bar, norm-wise (tests/test_cg_conv_ad.py)"""
    got, ref = np.asarray(got, f64), np.asarray(ref, f64)
    assert got.shape == ref.shape, what
    assert np.all(np.isfinite(got)), f"{what}: non-finite"
    err, scale = np.linalg.norm(got - ref), np.linalg.norm(ref)
    print(f"{what}: |got - ref| = {err:.3e}, |ref| = {scale:.3e}, ratio {err / max(scale, 1e-300):.2e}")
    assert err <= tol * scale, f"{what}: {err:.3e} > {tol:g} * {scale:.3e}"


def ptr(v):
    return None if v is None else ctypes.c_void_p(v.data_ptr())


def call_grad(lib, plan_t, x, we, dm, dx, dwe, Din, Dout, stream=None):
    from gnnmp import _lib
    job = _lib.NNConvGradJob(x, we, dm, dx, dwe)
    return lib.gnnmp_nn_conv_grad_f32(plan_t, ctypes.byref(job), Din, Dout, stream)


@pytest.fixture(scope="module")
def lib():
    import torch
    assert torch.cuda.is_available()
    from gnnmp import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def graph(lib):
    """the multigraph of tests/cg_conv_ref.py as a GNNGraph with 0-based int64 indices; its properties, and that both plans DO split the
    hub rows (the forward meets chunked rows, the gradient pass walks them whole)"""
    import gnnmp
    s, t = R.graph()
    R.assert_graph(s, t)
    g = gnnmp.GNNGraph(dev(s), dev(t), num_nodes=R.N_NODES, index_base=0)
    plan, plan_t = g.plan(False), g.plan_transposed(False)
    assert 600 > plan.long_thresh == plan_t.long_thresh and plan.n_long >= 1 and plan_t.n_long >= 1
    return g, s, t


def run_kernel(lib, g, case, Din, Dout, want_x=True, want_we=True):
    """(dx | None, dwe | None) of the export as numpy arrays; outputs start as NaN; `we` is not passed when dx is not wanted"""
    import torch
    x, we, dm = [dev(a) for a in case]
    dx = torch.full_like(x, float("nan")) if want_x else None
    dwe = torch.full_like(we, float("nan")) if want_we else None
    rc = call_grad(lib, g.plan_transposed(False).handle, ptr(x), ptr(we) if want_x else None, ptr(dm), ptr(dx), ptr(dwe), Din, Dout)
    assert rc == A.OK, lib.gnnmp_last_error()
    torch.cuda.synchronize()
    return tuple(None if v is None else v.cpu().numpy() for v in (dx, dwe))


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU 1: the kernel against float64
# ------------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("Din,Dout", R.KERNEL_SHAPES)
def test_kernel_against_float64(lib, graph, Din, Dout):
    """(1, 1): a single lane; (3, 5), (5, 16), (16, 4): tails in either dimension; (33, 20): five in-channel tiles, the last with one
    channel; (20, 70): 35 8-byte lanes; (64, 64): the workload; (3, 130), (2, 260): 65 lanes' worth of outputs, lane 0 owns two vectors.
    dx and dwe each within 1e-5, norm-wise, of float64; rows without out-edges written and zero; either output alone has the same bits"""
    g, s, t = graph
    case = R.kernel_case(Din, Dout)
    dx, dwe = run_kernel(lib, g, case, Din, Dout)
    dx_ref, dwe_ref = R.kernel_ref64(s, t, case, Din, Dout)
    close(dx, dx_ref, "dx")
    close(dwe, dwe_ref, "dwe")
    outdeg = np.bincount(s, minlength=R.N_NODES)
    assert (outdeg == 0).any() and not dx[outdeg == 0].any()
    only_x, none = run_kernel(lib, g, case, Din, Dout, want_we=False)
    assert none is None and np.array_equal(bits(only_x), bits(dx))
    none, only_w = run_kernel(lib, g, case, Din, Dout, want_x=False)
    assert none is None and np.array_equal(bits(only_w), bits(dwe))


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU 2: the layer
# ------------------------------------------------------------------------------------------------------------------------------------
def make_layer(shape, nn, W, b, sigma, aggr):
    import gnnmp
    nin, _, out = shape
    denses = []
    for Wn, bn, act in nn:
        d = gnnmp.Dense((Wn.shape[1], Wn.shape[0]), act)
        d.weight, d.bias = dev(Wn), dev(bn)
        denses.append(d)
    l = gnnmp.NNConv((nin, out), denses if len(denses) > 1 else denses[0], sigma, aggr=aggr, bias=b is not None)
    l.weight = dev(W)
    if b is not None:
        l.bias = dev(b)
    return l


def named_params(l):
    """[(name of the gradient, tensor)] in the order of nn_conv_ref.flat"""
    items = [("dW", l.weight)] + ([("db", l.bias)] if l.bias is not None else [])
    for i, d in enumerate(l.nn if isinstance(l.nn, list) else [l.nn]):
        items += [(f"nn{i}.dW", d.weight), (f"nn{i}.db", d.bias)]
    return items


def layer_grads(l, g, x, e, dy):
    """{y, dx, de, dW, db, nn<i>.dW, nn<i>.db} of nn_conv_ad as numpy arrays"""
    import torch
    import gnnmp
    xt, et = dev(x).requires_grad_(True), dev(e).requires_grad_(True)
    for _, p in named_params(l):
        p.requires_grad_(True)
        p.grad = None
    y = gnnmp.nn_conv_ad(l, g, xt, et)
    y.backward(dev(dy))
    torch.cuda.synchronize()
    res = dict(y=y.detach().cpu().numpy(), dx=xt.grad.cpu().numpy(), de=et.grad.cpu().numpy())
    res.update({k: p.grad.cpu().numpy() for k, p in named_params(l)})
    return res


@gpu
@pytest.mark.parametrize("shape,depth,sigma,aggr,bias", LAYER_CASES)
def test_layer_against_the_composition(graph, shape, depth, sigma, aggr, bias):
    """nn_conv_ad(...).backward(Δ): y, dx, de, dW, db and every parameter of nn within 1e-5 of the float64 composition; y bit-equal to
    gnnmp.nn_conv, with and without no_grad"""
    import torch
    import gnnmp
    g, s, t = graph
    x, e, nn, W, b, dy = R.layer_case(shape, depth)
    if not bias:
        b = None
    l = make_layer(shape, nn, W, b, sigma, aggr)
    got = layer_grads(l, g, x, e, dy)
    ref = R.grad64(s, t, R.N_NODES, x, e, nn, W, b, sigma, aggr, dy)
    want = R.flat(ref, bias)
    assert set(got) == {k for k, _ in want}
    for k, v in want:
        close(got[k], v, k)
    with torch.no_grad():
        y_plain = gnnmp.nn_conv(l, g, dev(x), dev(e))
        y_nograd = gnnmp.nn_conv_ad(l, g, dev(x), dev(e))
    assert not y_nograd.requires_grad
    assert np.array_equal(bits(got["y"]), bits(y_plain.cpu().numpy())) and np.array_equal(bits(y_nograd.cpu().numpy()), bits(got["y"]))


@gpu
def test_what_needs_no_gradient_gets_none(graph, monkeypatch):
    """requires_grad=False on x, on e, on nn's parameters, on all of them: their .grad stays None and the others are still within 1e-5 of
    the reference.  When neither e nor a parameter of nn needs a gradient the export is called without dwe: no E x out x in buffer"""
    import torch
    import gnnmp
    from gnnmp import backward_nn
    g, s, t = graph
    shape, depth, sigma, aggr = (5, 2, 5), 2, "relu", "mean"
    x, e, nn, W, b, dy = R.layer_case(shape, depth)
    full = dict(R.flat(R.grad64(s, t, R.N_NODES, x, e, nn, W, b, sigma, aggr, dy)))
    wanted = []
    inner = backward_nn.nn_rows_grad
    monkeypatch.setattr(backward_nn, "nn_rows_grad", lambda *a, **k: wanted.append((k["want_x"], k["want_we"])) or inner(*a, **k))
    nn_names = ("nn0.dW", "nn0.db", "nn1.dW", "nn1.db")
    every = ("dx", "de", "dW", "db") + nn_names
    for off in (("dx",), ("de",), nn_names, ("de",) + nn_names, every):
        l = make_layer(shape, nn, W, b, sigma, aggr)
        leaves = dict(dx=dev(x), de=dev(e), **dict(named_params(l)))
        for k in every:
            leaves[k].requires_grad_(k not in off)
        del wanted[:]
        y = gnnmp.nn_conv_ad(l, g, leaves["dx"], leaves["de"])
        if off == every:
            assert not y.requires_grad
            continue
        y.backward(dev(dy))
        torch.cuda.synchronize()
        assert wanted == [("dx" not in off, not set(("de",) + nn_names) <= set(off))], (off, wanted)
        for k in every:
            if k in off:
                assert leaves[k].grad is None, (off, k)
            else:
                close(leaves[k].grad.cpu().numpy(), full[k], f"{k} without {off}")


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU 3: the memory contract
# ------------------------------------------------------------------------------------------------------------------------------------
def contract_graph():
    s, t = R.graph()
    return A.Graph("nn", s + 1, t + 1, R.N_NODES)


def slab_arrays(case, want_x=True, want_we=True):
    x, we, dm = case
    arrs = [A.Arr("x", "in", x)] + ([A.Arr("we", "in", we)] if want_x else []) + [A.Arr("dm", "in", dm)]
    return arrs + ([A.Arr("dx", "out", shape=x.shape)] if want_x else []) + ([A.Arr("dwe", "out", shape=we.shape)] if want_we else [])


def slab_call(lib, slab, plan_t, Din, Dout, stream):
    p = lambda nm: slab.ptr(nm) if nm in slab.arrs else None      # noqa: E731
    return call_grad(lib, plan_t, p("x"), p("we"), p("dm"), p("dx"), p("dwe"), Din, Dout, stream)


def slab_want(s, t, case, Din, Dout, want_x=True, want_we=True):
    dx, dwe = R.kernel_ref64(s, t, case, Din, Dout)
    return {k: A.E(v) for k, v, w in (("dx", dx, want_x), ("dwe", dwe, want_we)) if w}


@gpu
@pytest.mark.parametrize("Din,Dout", [(8, 8), (3, 5)])
def test_memory_contract(lib, Din, Dout):
    """every element of dx and dwe written, no store before or after an array or into an input, with each array in turn shifted to 16-, 8-
    and 4-byte alignment ((8, 8): 16-byte lanes narrow to 8 and 4; (3, 5): 4-byte lanes throughout), on a side stream — the hub rows
    included.  Then once with dx = NULL (and no we) and once with dwe = NULL, each also with an array off alignment."""
    import torch
    side = torch.cuda.Stream()
    sp = ctypes.c_void_p(side.cuda_stream)
    plans = A.Plans(lib)
    s, t = R.graph()
    g = contract_graph()
    case = R.kernel_case(Din, Dout)
    try:
        plan_t = plans.get(A.Pl(g, T=True))
        names = [a.name for a in slab_arrays(case)]
        runs = [({}, True, True)] + [({nm: A.SHIFTS[a]}, True, True) for nm in names for a in ("a16", "a8", "a4")]
        runs += [({}, False, True), ({"dwe": 4}, False, True), ({}, True, False), ({"we": 8}, True, False)]
        for shifts, want_x, want_we in runs:
            slab = A.Slab(slab_arrays(case, want_x, want_we), "cuda", shifts)
            torch.cuda.synchronize()
            rc = slab_call(lib, slab, plan_t, Din, Dout, sp)
            torch.cuda.synchronize()
            assert rc == A.OK, (shifts, lib.gnnmp_last_error())
            problems = slab.check(slab_want(s, t, case, Din, Dout, want_x, want_we))
            assert not problems, (shifts, want_x, want_we, problems)
    finally:
        plans.close()


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU 4 and 5: capture, determinism, empty graphs
# ------------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("Din,Dout", [(8, 8), (3, 5)])
def test_the_export_records_into_a_hip_graph_without_an_eager_call(lib, Din, Dout):
    """recorded first (capture_error_mode = thread_local: a host wait or an allocation would be an error; the outputs still hold poison
    after the capture), then replayed twice with new values in the same buffers: each replay is bit-equal to an eager call on the same
    values, made afterwards"""
    import torch
    s, t = R.graph()
    g = contract_graph()
    cases = [R.kernel_case(Din, Dout, seed=sd) for sd in (100, 101)]
    assert not np.array_equal(cases[0][0], cases[1][0])
    side = torch.cuda.Stream()
    sp = ctypes.c_void_p(side.cuda_stream)
    plans = A.Plans(lib)
    try:
        plan_t = plans.get(A.Pl(g, T=True))
        slab = A.Slab(slab_arrays(cases[0]))
        graph = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            graph.capture_begin(capture_error_mode="thread_local")
            try:
                rc = slab_call(lib, slab, plan_t, Din, Dout, sp)
            finally:
                graph.capture_end()
        torch.cuda.synchronize()
        assert rc == A.OK, lib.gnnmp_last_error()
        assert not slab.check({}, untouched=True), "work ran while the call was being recorded"
        inputs = lambda case: dict(zip(("x", "we", "dm"), case))      # noqa: E731
        replayed = []
        for case in cases:
            slab.reload(inputs(case))
            graph.replay()
            torch.cuda.synchronize()
            assert not slab.check(slab_want(s, t, case, Din, Dout))
            replayed.append(slab.outputs())
        for case, rep in zip(cases, replayed):
            slab.reload(inputs(case))
            torch.cuda.synchronize()
            assert slab_call(lib, slab, plan_t, Din, Dout, sp) == A.OK, lib.gnnmp_last_error()
            torch.cuda.synchronize()
            eager = slab.outputs()
            assert all(np.array_equal(eager[k], rep[k]) for k in eager)
        del graph
    finally:
        plans.close()


@gpu
def test_two_calls_give_equal_bits(lib, graph):
    g, s, t = graph
    for Din, Dout in ((64, 64), (33, 20), (3, 5)):
        case = R.kernel_case(Din, Dout)
        first, again = run_kernel(lib, g, case, Din, Dout), run_kernel(lib, g, case, Din, Dout)
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(first, again)), (Din, Dout)
    shape, depth = (16, 8, 16), 2
    x, e, nn, W, b, dy = R.layer_case(shape, depth)
    l = make_layer(shape, nn, W, b, "relu", "mean")
    first, again = layer_grads(l, g, x, e, dy), layer_grads(l, g, x, e, dy)
    for k in first:
        assert np.array_equal(bits(first[k]), bits(again[k])), k


@gpu
def test_empty_graphs(lib):
    """N = 0 launches nothing (the plan's head says so); E = 0 with N > 0 writes zeros to dx and touches no row of dwe"""
    import torch
    import gnnmp
    none = _FakePlan(n_src=0, n_dst=0, n_edges=0, n_total=0)
    assert _grad(lib, ctypes.addressof(none)) == A.OK
    n, Din, Dout = 9, 11, 6
    nothing = np.zeros(0, np.int64)
    g = gnnmp.GNNGraph(dev(nothing), dev(nothing), num_nodes=n, index_base=0)
    rng = np.random.default_rng(0)
    x, dm = dev(rng.standard_normal((n, Din)).astype(f32)), dev(rng.standard_normal((n, Dout)).astype(f32))
    we = torch.zeros((1, Dout * Din), dtype=torch.float32, device="cuda")      # E = 0: no row of it is read, no row of dwe written
    for want_x, want_we in ((True, True), (True, False), (False, True)):
        dx = torch.full_like(x, float("nan")) if want_x else None
        dwe = torch.full_like(we, float("nan")) if want_we else None
        rc = call_grad(lib, g.plan_transposed(False).handle, ptr(x), ptr(we) if want_x else None, ptr(dm), ptr(dx), ptr(dwe), Din, Dout)
        assert rc == A.OK, lib.gnnmp_last_error()
        torch.cuda.synchronize()
        assert dwe is None or bool(torch.isnan(dwe).all())
        assert dx is None or not dx.cpu().numpy().any()


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU 6: what nn_conv_ad refuses
# ------------------------------------------------------------------------------------------------------------------------------------
@gpu
def test_nn_conv_ad_refuses_by_name(graph):
    import gnnmp
    g, _, _ = graph
    shape = (5, 2, 5)
    x, e, nn, W, b, _ = R.layer_case(shape, 1)
    l = make_layer(shape, nn, W, b, None, "+")
    xt, et = dev(x), dev(e)
    with pytest.raises(NotImplementedError, match="bipartite"):
        gnnmp.nn_conv_ad(l, g, (xt, xt), et)
    for aggr in ("max", "min"):
        with pytest.raises(NotImplementedError, match=f"aggr = '{aggr}'"):
            gnnmp.nn_conv_ad(make_layer(shape, nn, W, b, None, aggr), g, xt, et)
    with pytest.raises(ValueError, match="x has 4 features, the layer was built for 5"):
        gnnmp.nn_conv_ad(l, g, xt[:, :4].contiguous(), et)
    narrow = make_layer(shape, [(nn[0][0][:20].copy(), nn[0][1][:20].copy(), None)], W, b, None, "+")
    with pytest.raises(ValueError, match=r"nn\(e\) has 20 features, the layer needs out \* in = 25"):
        gnnmp.nn_conv_ad(narrow, g, xt, et)
    other = make_layer(shape, nn, W, b, None, "+")
    other.nn = [other.nn, lambda v: v]
    with pytest.raises(TypeError, match="layer 1 of nn is a function"):
        gnnmp.nn_conv_ad(other, g, xt, et)
    import torch
    tanh = make_layer(shape, [(nn[0][0], nn[0][1], torch.tanh)], W, b, None, "+")      # dense_ad's own refusal, in the backward
    y = gnnmp.nn_conv_ad(tanh, g, xt, et.requires_grad_(True))
    with pytest.raises(ValueError, match="the HIP adjoints cover"):
        y.sum().backward()


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU 7: a small MPNN step
# ------------------------------------------------------------------------------------------------------------------------------------
@gpu
def test_a_small_mpnn_step():
    """radius_graph(pos) -> e = 4 Gaussian basis functions of the edge length (torch; a leaf that requires a gradient) -> two
    NNConv(8 => 8, nn = [Dense(4 => 16, relu), Dense(16 => 64)], relu; aggr = mean) -> global_pool_ad mean; 4 clouds of 48 points in the unit
    cube, loss = Σ pooled .* R: every parameter gradient, dx and de against the float64 chain on the edge list the device built.  The
    radius gives every cloud a mean degree of at least 3 and no node more than 12 neighbours (isolated nodes are fine: mean of nothing is
    0); no relu pre-activation of the float64 chain is closer than 1e-5 to the kink."""
    import torch
    import gnnmp
    from gnnmp.backward import global_pool_ad
    pos, gi, x, layers, Rm = R.mpnn_case()
    c = R.MPNN
    n = len(pos)
    pd = dev(pos)
    g = gnnmp.radius_graph(pd, c["radius"], graph_indicator=dev(gi + 1))
    s, t = g.s.cpu().numpy() - 1, g.t.cpu().numpy() - 1
    assert np.array_equal(gi[s], gi[t]) and not (s == t).any()
    deg = np.bincount(t, minlength=n)
    per_cloud = deg.reshape(c["clouds"], c["pts"]).mean(axis=1)
    print(f"radius graph: {len(s)} edges, mean degree per cloud {per_cloud}, min {deg.min()}, max {deg.max()}")
    assert per_cloud.min() >= 3 and deg.max() <= 12
    length = (pd[g.s - 1] - pd[g.t - 1]).norm(dim=1, keepdim=True)
    mu = torch.linspace(0.0, c["radius"], c["ein"], device="cuda")
    et = torch.exp(-((length - mu) / (c["radius"] / c["ein"])) ** 2).detach().contiguous().requires_grad_(True)
    ls = [make_layer((c["nin"], c["ein"], c["nin"]), nn, W, b, "relu", "mean") for nn, W, b in layers]
    for l in ls:
        for _, p in named_params(l):
            p.requires_grad_(True)
    xt = dev(x).requires_grad_(True)
    h1 = gnnmp.nn_conv_ad(ls[0], g, xt, et)
    h2 = gnnmp.nn_conv_ad(ls[1], g, h1, et)
    pooled = global_pool_ad(gnnmp.GlobalPool("mean"), g, h2)
    (pooled * dev(Rm)).sum().backward()
    torch.cuda.synchronize()
    e = et.detach().cpu().numpy()
    h2_ref, grads, dx_ref, de_ref, kink = R.mpnn_grad64(s, t, gi, x, e, layers, Rm)
    print(f"smallest |relu pre-activation| {kink:.3e}")
    assert kink >= 1e-5
    close(h2.detach().cpu().numpy(), h2_ref, "h2")
    for i, (l, ref) in enumerate(zip(ls, grads)):
        want = dict(R.flat(ref))
        for k, p in named_params(l):
            close(p.grad.cpu().numpy(), want[k], f"{k} of layer {i + 1}")
    close(xt.grad.cpu().numpy(), dx_ref, "dx")
    close(et.grad.cpu().numpy(), de_ref, "de")
