"""cg_conv_ad: CGConv trained on the fused gated-message adjoint (csrc/cg_grad.hip; include/gnnmp.h states the arithmetic).

Without a GPU: the export exists in header, SYMBOLS and library and takes const plans and a const host record; every refusal of the header
comes before any HIP call; the float64 gradient reference (tests/cg_conv_ref.py) agrees with central finite differences for all four
activations; the operands of every GPU case keep the float32 restatement within 2e-6 of float64 and, for relu, away from the kink.

On the GPU: dfs_i, dfs_j, dfs_e of the export within 1e-5 of float64 at every lane width, tail and tile count, on a multigraph with self
loops, repeated edges, a row without in-edges, a row without out-edges and a hub destination and source of 600 edges; the layer's y, dx, de,
dWf, dWs, dbf, dbs within 1e-5 of the reference's composition, y bit-equal to gnnmp.cg_conv; every output element written and nothing else
(the slab of tests/abi_cases.py) at any pointer alignment; the export recorded into a HIP graph without an eager call first; two calls give
equal bits; empty graphs; the refusals of cg_conv_ad; a small CGCNN step on a device-built radius graph."""
import ctypes
import itertools
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_cases as A  # noqa: E402
import cg_conv_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRAD = "gnnmp_cg_conv_grad_f32"
gpu = pytest.mark.gpu
f32, f64 = np.float32, np.float64
FIELDS = ("fs_i", "fs_j", "fs_e", "dy", "dfs_i", "dfs_j", "dfs_e", "act")


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
    assert "} gnnmp_cg_conv_grad_t;" in header
    assert "GNNlib/src/layers/conv.jl:304-333" in header[:internal]
    assert "tests/test_cg_conv_ad.py" in header[:header.index("#ifndef GNNMP_H")]           # the Conventions paragraph: what is tested
    assert callable(gnnmp.cg_conv_ad)


def test_the_export_takes_const_plans_and_a_const_host_record():
    """device pointers travel in a const host record: the table of tests/abi_cases.py owes no case, this file carries the memory-contract
    and capture checks itself.  The ctypes record has the layout of the header's struct."""
    import re
    from gnnmp import _lib
    decls, _ = A.parse_header()
    assert GRAD not in A.must_be_covered(decls, _lib.SYMBOLS)
    assert [p[0] for p in decls[GRAD]] == ["plan", "plan_t", "job", "C", "stream"]
    for pname, is_ptr, is_const, _ in decls[GRAD]:
        assert is_const or not is_ptr, pname
    header = open(os.path.join(ROOT, "include", "gnnmp.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} gnnmp_cg_conv_grad_t;", header).group(1)
    body = re.sub(r"/\*.*?\*/", " ", body, flags=re.S)
    fields, off, offsets = [], 0, []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        is_ptr = "*" in decl
        names = [n.strip().lstrip("*") for n in re.sub(r"^(const\s+)?(float|int)\s+", "", decl).split(",")]
        for nme in names:
            size = 8 if is_ptr else 4
            off = (off + size - 1) // size * size
            fields.append(nme)
            offsets.append(off)
            off += size
    assert tuple(fields) == FIELDS
    assert [getattr(_lib.CGConvGradJob, f).offset for f in FIELDS] == offsets == [0, 8, 16, 24, 32, 40, 48, 56]
    assert ctypes.sizeof(_lib.CGConvGradJob) == 64


P = lambda v: ctypes.c_void_p(0x1000 * v) if v else None      # never dereferenced: the call must refuse first  # noqa: E731


class _FakePlan(ctypes.Structure):
    """the head of csrc/common.h's gnnmp_graph {int64 n_src, n_dst, n_edges, n_total; ...}: all the refusals read of a plan"""
    _fields_ = [("n_src", ctypes.c_int64), ("n_dst", ctypes.c_int64), ("n_edges", ctypes.c_int64), ("n_total", ctypes.c_int64),
                ("tail", ctypes.c_char * 1024)]


def _grad(lib, plan, plan_t, job=True, fs_i=1, fs_j=2, fs_e=3, dy=4, dfs_i=5, dfs_j=6, dfs_e=7, act=0, C=4):
    from gnnmp import _lib
    j = _lib.CGConvGradJob(P(fs_i), P(fs_j), P(fs_e), P(dy), P(dfs_i), P(dfs_j), P(dfs_e), act)
    return lib.gnnmp_cg_conv_grad_f32(plan, plan_t, ctypes.byref(j) if job else None, C, None)


def test_argument_validation_needs_no_gpu():
    """every refusal of the header comes before the first HIP call: on a machine without a device, on pointers that are not memory"""
    from gnnmp import _lib
    lib = _lib.load()
    EINVAL, err = _lib.EINVAL, lib.gnnmp_last_error
    sq, sq_t = _FakePlan(n_src=5, n_dst=5, n_edges=7, n_total=7), _FakePlan(n_src=5, n_dst=5, n_edges=7, n_total=7)
    pl, pt = ctypes.addressof(sq), ctypes.addressof(sq_t)
    assert _grad(lib, None, pt) == EINVAL and b"null plan" in err()
    assert _grad(lib, pl, None) == EINVAL and b"null plan_t" in err()
    assert _grad(lib, pl, pt, job=False) == EINVAL and b"null job" in err()
    for name in ("fs_i", "fs_j", "dy", "dfs_i", "dfs_j"):
        assert _grad(lib, pl, pt, **{name: None}) == EINVAL and f"null {name}".encode() in err(), name
    assert _grad(lib, pl, pt, fs_e=None) == EINVAL and b"dfs_e without fs_e" in err()
    for C in (0, -3, (1 << 19) + 1, 2 ** 40):
        assert _grad(lib, pl, pt, C=C) == EINVAL and b"bad C" in err(), C
    for act in (-1, 4, 17):                                      # swish and beyond: not an activation of CGConv
        assert _grad(lib, pl, pt, act=act) == EINVAL and b"bad act" in err(), act
    rect = _FakePlan(n_src=9, n_dst=5, n_edges=7, n_total=7)
    assert _grad(lib, ctypes.addressof(rect), pt) == EINVAL and b"not square" in err()
    tall = _FakePlan(n_src=6, n_dst=6, n_edges=7, n_total=7)
    assert _grad(lib, pl, ctypes.addressof(tall)) == EINVAL and b"the transposed plan has 6 rows, the plan 5" in err()
    more = _FakePlan(n_src=5, n_dst=5, n_edges=8, n_total=8)
    assert _grad(lib, pl, ctypes.addressof(more)) == EINVAL and b"the transposed plan has 8 edges, the plan 7" in err()
    loops, loops_t = _FakePlan(n_src=5, n_dst=5, n_edges=7, n_total=12), _FakePlan(n_src=5, n_dst=5, n_edges=7, n_total=12)
    assert _grad(lib, ctypes.addressof(loops), ctypes.addressof(loops_t)) == EINVAL and b"self loops" in err()
    # N = 0 launches nothing: accepted on a machine without a device — with and without the optional pointers
    none = _FakePlan(n_src=0, n_dst=0, n_edges=0, n_total=0)
    assert _grad(lib, ctypes.addressof(none), ctypes.addressof(none)) == _lib.OK
    assert _grad(lib, ctypes.addressof(none), ctypes.addressof(none), fs_e=None, dfs_e=None) == _lib.OK
    assert _grad(lib, ctypes.addressof(none), ctypes.addressof(none), dfs_e=None, C=1 << 19, act=3) == _lib.OK


# ------------------------------------------------------------------------------------------------------------------------------------
# CPU: the references
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("name", R.ACTS)
@pytest.mark.parametrize("nin", [4, 5])
def test_reference_gradient_agrees_with_finite_differences(nin, name, residual):
    """central differences of the float64 composition: n = 30, E = 200, ein = 3, C = 5, h = 1e-6 (nin = 4: the residual is asked for but
    not applied, nin != out; nin = 5: it is applied); relu's inputs are kept off the kink"""
    h = 1e-6
    s, t, n, x, e, Wf, Ws, bf, bs, dy = R.fd_case(nin, name)
    ref = R.grad64(s, t, n, x, e, Wf, Ws, bf, bs, name, residual, dy)
    if name == "relu":
        assert np.abs(ref["sp"]).min() > 100 * h
    loss = lambda: float((R.compose(s, t, n, x, e, Wf, Ws, bf, bs, name, residual)[3] * dy).sum())      # noqa: E731
    for arr, what in ((x, "dx"), (e, "de"), (Wf, "dWf"), (Ws, "dWs"), (bf, "dbf"), (bs, "dbs")):
        g = ref[what]
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


def test_the_split_formulation_is_the_composition():
    """in float64 the header's split formulation and the reference's composition agree to rounding, with and without e, bias, residual"""
    s, t = R.graph()
    R.assert_graph(s, t)
    for shape, name in zip(R.LAYER_SHAPES, R.ACTS):
        x, e, Wf, Ws, bf, bs, dy = R.layer_case(shape, name)
        for residual, bias in itertools.product((False, True), repeat=2):
            b = (bf, bs) if bias else (None, None)
            got = R.layer(s, t, R.N_NODES, x, e, Wf, Ws, *b, name, residual, dy, f64)
            ref = R.grad64(s, t, R.N_NODES, x, e, Wf, Ws, *b, name, residual, dy)
            for k in R.WHAT:
                if ref[k] is not None:
                    assert R.rel(got[k], ref[k]) < 1e-13, (shape, name, residual, bias, k)


KERNEL_CASES = list(itertools.product(R.KERNEL_CS, R.ACTS, (False, True)))
LAYER_CASES = list(itertools.product(R.LAYER_SHAPES, R.ACTS, (False, True), (False, True)))      # shape, act, residual, bias


def _assert_conditioned(what, cond, name):
    worst, ratio = cond
    assert worst <= R.COND, f"{what}: the float32 restatement is {worst:.2e} from float64 (bound {R.COND:g})"
    if name == "relu":
        assert ratio >= R.MARGIN, f"{what}: the smallest |s_k| is only {ratio:.1f} x the float32-float64 deviation of s_k"


@pytest.mark.parametrize("C,name,with_e", KERNEL_CASES)
def test_the_kernel_cases_are_well_conditioned(C, name, with_e):
    """THE CONDITION ON THE INPUTS, not a measurement: dfs_i, dfs_j, dfs_e evaluated in float32 by the header's formulas are within 2e-6,
    norm-wise, of float64 — a fifth of the 1e-5 bar; the rest is left to the hardware exp / rcp / log — and relu's kink is far away"""
    s, t = R.graph()
    _assert_conditioned("kernel case", R.kernel_condition(s, t, R.kernel_case(C, name, with_e), C, name), name)


@pytest.mark.parametrize("shape,name,residual,bias", LAYER_CASES)
def test_the_layer_cases_are_well_conditioned(shape, name, residual, bias):
    s, t = R.graph()
    _assert_conditioned("layer case", R.layer_condition(s, t, R.layer_case(shape, name), name, residual, bias), name)


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU helpers
# ------------------------------------------------------------------------------------------------------------------------------------
def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def close(got, ref, what, tol=1e-5):
    """the project's parity bar, norm-wise (tests/test_edge_conv_ad.py)"""
    got, ref = np.asarray(got, f64), np.asarray(ref, f64)
    assert got.shape == ref.shape, what
    assert np.all(np.isfinite(got)), f"{what}: non-finite"
    err, scale = np.linalg.norm(got - ref), np.linalg.norm(ref)
    print(f"{what}: |got - ref| = {err:.3e}, |ref| = {scale:.3e}, ratio {err / max(scale, 1e-300):.2e}")
    assert err <= tol * scale, f"{what}: {err:.3e} > {tol:g} * {scale:.3e}"


def ptr(v):
    return None if v is None else ctypes.c_void_p(v.data_ptr())


def call_grad(lib, plan, plan_t, fs_i, fs_j, fs_e, dy, dfs_i, dfs_j, dfs_e, act, C, stream=None):
    from gnnmp import _lib
    job = _lib.CGConvGradJob(fs_i, fs_j, fs_e, dy, dfs_i, dfs_j, dfs_e, act)
    return lib.gnnmp_cg_conv_grad_f32(plan, plan_t, ctypes.byref(job), C, stream)


@pytest.fixture(scope="module")
def lib():
    import torch
    assert torch.cuda.is_available()
    from gnnmp import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def graph(lib):
    """the multigraph of tests/cg_conv_ref.py as a GNNGraph with 0-based int64 indices; its properties, and that both plans DO split the
    hub rows (the forward meets chunked rows, the gradient passes walk them whole)"""
    import gnnmp
    s, t = R.graph()
    R.assert_graph(s, t)
    g = gnnmp.GNNGraph(dev(s), dev(t), num_nodes=R.N_NODES, index_base=0)
    plan, plan_t = g.plan(False), g.plan_transposed(False)
    assert R.HUB > plan.long_thresh == plan_t.long_thresh and plan.n_long >= 1 and plan_t.n_long >= 1
    return g, s, t


def run_kernel(lib, g, case, C, name, want_e=True):
    """(dfs_i, dfs_j, dfs_e | None) of the export as numpy arrays; outputs start as NaN"""
    import torch
    fs_i, fs_j, fs_e, dy = [None if a is None else dev(a) for a in case]
    nan = lambda like: torch.full_like(like, float("nan"))      # noqa: E731
    di, dj = nan(fs_i), nan(fs_j)
    de = nan(fs_e) if (fs_e is not None and want_e) else None
    rc = call_grad(lib, g.plan(False).handle, g.plan_transposed(False).handle, ptr(fs_i), ptr(fs_j), ptr(fs_e), ptr(dy), ptr(di), ptr(dj),
                   ptr(de), R.ACT_CODE[name], C)
    assert rc == A.OK, lib.gnnmp_last_error()
    torch.cuda.synchronize()
    return tuple(None if v is None else v.cpu().numpy() for v in (di, dj, de))


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU 1: the kernels against float64
# ------------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("C,name,with_e", KERNEL_CASES)
def test_kernel_against_float64(lib, graph, C, name, with_e):
    """C = 1, 3: 4-byte lanes; 6: 8-byte lanes; 8, 64: 16-byte lanes; 260: a second feature tile with one active lane.  The export is
    called directly on fs_i, fs_j, fs_e, Δ built on the host; dfs_i, dfs_j, dfs_e within 1e-5, norm-wise, of the float64 values"""
    g, s, t = graph
    case = R.kernel_case(C, name, with_e)
    got = run_kernel(lib, g, case, C, name)
    ref = R.kernel_ref64(s, t, case, C, name)
    for what, a, b in zip(("dfs_i", "dfs_j", "dfs_e"), got, ref):
        assert (a is None) == (b is None), what
        if a is not None:
            close(a, b, what)
    indeg, outdeg = np.bincount(t, minlength=R.N_NODES), np.bincount(s, minlength=R.N_NODES)
    assert not got[0][indeg == 0].any() and not got[1][outdeg == 0].any()      # rows without edges: written, zero
    if with_e:      # dfs_e not wanted: the node-level outputs have the same bits
        again = run_kernel(lib, g, case, C, name, want_e=False)
        assert again[2] is None and np.array_equal(bits(again[0]), bits(got[0])) and np.array_equal(bits(again[1]), bits(got[1]))


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU 2: the layer
# ------------------------------------------------------------------------------------------------------------------------------------
def make_layer(shape, name, residual, Wf, Ws, bf, bs):
    import gnnmp
    nin, ein, out = shape
    l = gnnmp.CGConv(((nin, ein), out), name, residual=residual, bias=bf is not None)
    l.dense_f_weight, l.dense_s_weight = dev(Wf), dev(Ws)
    if bf is not None:
        l.dense_f_bias, l.dense_s_bias = dev(bf), dev(bs)
    return l


def params(l):
    return [p for p in (l.dense_f_weight, l.dense_s_weight, l.dense_f_bias, l.dense_s_bias) if p is not None]


def layer_grads(l, g, x, e, dy):
    """dict(y, dx, de, dWf, dWs, dbf, dbs) of cg_conv_ad as numpy arrays (None where the layer has no such operand)"""
    import torch
    import gnnmp
    xt = dev(x).requires_grad_(True)
    et = None if e is None else dev(e).requires_grad_(True)
    for p in params(l):
        p.requires_grad_(True)
        p.grad = None
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        y = gnnmp.cg_conv_ad(l, g, xt, et)
    y.backward(dev(dy))
    torch.cuda.synchronize()
    np_ = lambda v: None if v is None else v.detach().cpu().numpy()      # noqa: E731
    grad = lambda p: None if p is None else np_(p.grad)      # noqa: E731
    return dict(y=np_(y), dx=grad(xt), de=grad(et), dWf=grad(l.dense_f_weight), dWs=grad(l.dense_s_weight), dbf=grad(l.dense_f_bias),
                dbs=grad(l.dense_s_bias))


@gpu
@pytest.mark.parametrize("shape,name,residual,bias", LAYER_CASES)
def test_layer_against_the_composition(graph, shape, name, residual, bias):
    """cg_conv_ad(...).backward(Δ): y, dx, de, dWf, dWs, dbf, dbs within 1e-5 of the float64 composition; y bit-equal to gnnmp.cg_conv"""
    import torch
    import gnnmp
    g, s, t = graph
    x, e, Wf, Ws, bf, bs, dy = R.layer_case(shape, name)
    if not bias:
        bf = bs = None
    l = make_layer(shape, name, residual, Wf, Ws, bf, bs)
    got = layer_grads(l, g, x, e, dy)
    ref = R.grad64(s, t, R.N_NODES, x, e, Wf, Ws, bf, bs, name, residual, dy)
    for k in R.WHAT:
        if k in ("dbf", "dbs") and not bias or k == "de" and e is None:
            assert got[k] is None, k
        else:
            close(got[k], ref[k], k)
    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        y_plain = gnnmp.cg_conv(l, g, dev(x), None if e is None else dev(e))
        y_nograd = gnnmp.cg_conv_ad(l, g, dev(x), None if e is None else dev(e))
    assert not y_nograd.requires_grad
    assert np.array_equal(bits(got["y"]), bits(y_plain.cpu().numpy())) and np.array_equal(bits(y_nograd.cpu().numpy()), bits(got["y"]))


@gpu
def test_what_needs_no_gradient_gets_none(graph):
    """requires_grad=False on a parameter or an input: its .grad stays None; the others are still within 1e-5 of the reference (what is
    not needed is not computed, so the dense adjoints may take another route: equal bits are not owed)"""
    import torch
    import gnnmp
    g, s, t = graph
    shape, name = (6, 3, 6), "softplus"
    x, e, Wf, Ws, bf, bs, dy = R.layer_case(shape, name)
    full = R.grad64(s, t, R.N_NODES, x, e, Wf, Ws, bf, bs, name, True, dy)
    names = ("dx", "de", "dWf", "dWs", "dbf", "dbs")
    for off in (("dx",), ("de",), ("dWf", "dbs"), ("de", "dWf", "dWs"), ("dx", "de", "dWf", "dWs", "dbf", "dbs")):
        l = make_layer(shape, name, True, Wf, Ws, bf, bs)
        leaves = dict(dx=dev(x), de=dev(e), dWf=l.dense_f_weight, dWs=l.dense_s_weight, dbf=l.dense_f_bias, dbs=l.dense_s_bias)
        for k in names:
            leaves[k].requires_grad_(k not in off)
        y = gnnmp.cg_conv_ad(l, g, leaves["dx"], leaves["de"])
        if len(off) == len(names):
            assert not y.requires_grad
            continue
        y.backward(dev(dy))
        torch.cuda.synchronize()
        for k in names:
            if k in off:
                assert leaves[k].grad is None, (off, k)
            else:
                close(leaves[k].grad.cpu().numpy(), full[k], f"{k} without {off}")


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU 3: the memory contract
# ------------------------------------------------------------------------------------------------------------------------------------
def contract_graph():
    s, t = R.graph()
    return A.Graph("cg", s + 1, t + 1, R.N_NODES)


def slab_arrays(case, with_e, want_e):
    fs_i, fs_j, fs_e, dy = case
    arrs = [A.Arr("fs_i", "in", fs_i), A.Arr("fs_j", "in", fs_j)] + ([A.Arr("fs_e", "in", fs_e)] if with_e else [])
    arrs += [A.Arr("dy", "in", dy), A.Arr("dfs_i", "out", shape=fs_i.shape), A.Arr("dfs_j", "out", shape=fs_j.shape)]
    return arrs + ([A.Arr("dfs_e", "out", shape=fs_e.shape)] if with_e and want_e else [])


def slab_call(lib, slab, plan, plan_t, name, C, stream):
    p = lambda nm: slab.ptr(nm) if nm in slab.arrs else None      # noqa: E731
    return call_grad(lib, plan, plan_t, p("fs_i"), p("fs_j"), p("fs_e"), p("dy"), p("dfs_i"), p("dfs_j"), p("dfs_e"), R.ACT_CODE[name], C, stream)


def slab_want(s, t, case, with_e, want_e, C, name):
    di, dj, de = R.kernel_ref64(s, t, case, C, name)
    want = {"dfs_i": A.E(di), "dfs_j": A.E(dj)}
    if with_e and want_e:
        want["dfs_e"] = A.E(de)
    return want


@gpu
@pytest.mark.parametrize("with_e", [False, True], ids=["no_e", "e"])
@pytest.mark.parametrize("C", [8, 6])
def test_memory_contract(lib, C, with_e):
    """every element of dfs_i, dfs_j, dfs_e written, no store before or after an array or into an input, with each array in turn shifted
    to 16-, 8- and 4-byte alignment (C = 8: 16-byte lanes narrow to 8 and 4; C = 6: 8-byte lanes narrow to 4), on a side stream — the hub
    rows included.  With edge features also once without dfs_e."""
    import torch
    side = torch.cuda.Stream()
    sp = ctypes.c_void_p(side.cuda_stream)
    plans = A.Plans(lib)
    s, t = R.graph()
    g = contract_graph()
    try:
        plan, plan_t = plans.get(A.Pl(g)), plans.get(A.Pl(g, T=True))
        names = [a.name for a in slab_arrays(R.kernel_case(C, "identity", with_e), with_e, True)]
        runs = [({}, True)] + [({nm: A.SHIFTS[a]}, True) for nm in names for a in ("a16", "a8", "a4")]
        if with_e:
            runs += [({}, False), ({"fs_e": 4}, False)]
        for k, (shifts, want_e) in enumerate(runs):
            name = R.ACTS[k % 4]
            case = R.kernel_case(C, name, with_e)
            slab = A.Slab(slab_arrays(case, with_e, want_e), "cuda", shifts)
            torch.cuda.synchronize()
            rc = slab_call(lib, slab, plan, plan_t, name, C, sp)
            torch.cuda.synchronize()
            assert rc == A.OK, (shifts, lib.gnnmp_last_error())
            problems = slab.check(slab_want(s, t, case, with_e, want_e, C, name))
            assert not problems, (name, shifts, want_e, problems)
    finally:
        plans.close()


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU 4 and 5: capture, determinism, empty graphs
# ------------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name,with_e", [("softplus", True), ("tanh", False)])
def test_the_export_records_into_a_hip_graph_without_an_eager_call(lib, name, with_e):
    """recorded first (capture_error_mode = thread_local: a host wait or an allocation would be an error; the outputs still hold poison
    after the capture), then replayed twice with new values in the same buffers: each replay is bit-equal to an eager call on the same
    values, made afterwards"""
    import torch
    C = 8
    s, t = R.graph()
    g = contract_graph()
    cases = [R.kernel_case(C, name, with_e, seed=sd) for sd in (100, 101)]
    assert not np.array_equal(cases[0][0], cases[1][0])
    side = torch.cuda.Stream()
    sp = ctypes.c_void_p(side.cuda_stream)
    plans = A.Plans(lib)
    try:
        plan, plan_t = plans.get(A.Pl(g)), plans.get(A.Pl(g, T=True))
        slab = A.Slab(slab_arrays(cases[0], with_e, True))
        graph = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            graph.capture_begin(capture_error_mode="thread_local")
            try:
                rc = slab_call(lib, slab, plan, plan_t, name, C, sp)
            finally:
                graph.capture_end()
        torch.cuda.synchronize()
        assert rc == A.OK, lib.gnnmp_last_error()
        assert not slab.check({}, untouched=True), "work ran while the call was being recorded"
        inputs = lambda case: {k: v for k, v in zip(("fs_i", "fs_j", "fs_e", "dy"), case) if v is not None}      # noqa: E731
        replayed = []
        for case in cases:
            slab.reload(inputs(case))
            graph.replay()
            torch.cuda.synchronize()
            assert not slab.check(slab_want(s, t, case, with_e, True, C, name))
            replayed.append(slab.outputs())
        for case, rep in zip(cases, replayed):
            slab.reload(inputs(case))
            torch.cuda.synchronize()
            assert slab_call(lib, slab, plan, plan_t, name, C, sp) == A.OK, lib.gnnmp_last_error()
            torch.cuda.synchronize()
            eager = slab.outputs()
            assert all(np.array_equal(eager[k], rep[k]) for k in eager)
        del graph
    finally:
        plans.close()


@gpu
def test_two_calls_give_equal_bits(lib, graph):
    g, _, _ = graph
    for C, name in ((64, "softplus"), (6, "tanh"), (3, "relu")):
        case = R.kernel_case(C, name, True)
        first, again = run_kernel(lib, g, case, C, name), run_kernel(lib, g, case, C, name)
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(first, again)), (C, name)
    shape, name = (64, 16, 64), "softplus"
    x, e, Wf, Ws, bf, bs, dy = R.layer_case(shape, name)
    l = make_layer(shape, name, True, Wf, Ws, bf, bs)
    first, again = layer_grads(l, g, x, e, dy), layer_grads(l, g, x, e, dy)
    for k in R.WHAT:
        assert np.array_equal(bits(first[k]), bits(again[k])), k


@gpu
def test_empty_graphs(lib):
    """N = 0 launches nothing (the plan's head says so); E = 0 with N > 0 writes zeros everywhere"""
    import torch
    import gnnmp
    none = _FakePlan(n_src=0, n_dst=0, n_edges=0, n_total=0)
    assert _grad(lib, ctypes.addressof(none), ctypes.addressof(none)) == A.OK
    n, C = 9, 6
    nothing = np.zeros(0, np.int64)
    g = gnnmp.GNNGraph(dev(nothing), dev(nothing), num_nodes=n, index_base=0)
    rng = np.random.default_rng(0)
    fs_i, fs_j, dy = [dev(rng.standard_normal(shape).astype(f32)) for shape in ((n, 2 * C), (n, 2 * C), (n, C))]
    fs_e = torch.zeros((1, 2 * C), dtype=torch.float32, device="cuda")      # E = 0: no row of it is read, no row of dfs_e written
    for with_e in (False, True):
        di, dj = torch.full_like(fs_i, float("nan")), torch.full_like(fs_j, float("nan"))
        de = torch.full_like(fs_e, float("nan")) if with_e else None
        rc = call_grad(lib, g.plan(False).handle, g.plan_transposed(False).handle, ptr(fs_i), ptr(fs_j), ptr(fs_e if with_e else None), ptr(dy),
                       ptr(di), ptr(dj), ptr(de), R.ACT_CODE["softplus"], C)
        assert rc == A.OK, lib.gnnmp_last_error()
        torch.cuda.synchronize()
        assert de is None or bool(torch.isnan(de).all())
        assert not di.cpu().numpy().any() and not dj.cpu().numpy().any()


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU 6: what cg_conv_ad refuses
# ------------------------------------------------------------------------------------------------------------------------------------
@gpu
def test_cg_conv_ad_refuses_by_name(graph):
    import gnnmp
    g, _, _ = graph
    shape, name = (6, 3, 6), "softplus"
    x, e, Wf, Ws, bf, bs, _ = R.layer_case(shape, name)
    l = make_layer(shape, name, False, Wf, Ws, bf, bs)
    xt, et = dev(x), dev(e)
    with pytest.raises(NotImplementedError, match="bipartite"):
        gnnmp.cg_conv_ad(l, g, (xt, xt), et)
    with pytest.raises(ValueError, match="e has 2 features, the layer was built for 3"):
        gnnmp.cg_conv_ad(l, g, xt, et[:, :2].contiguous())
    with pytest.raises(ValueError, match="built with edge features"):
        gnnmp.cg_conv_ad(l, g, xt)
    plain = make_layer((6, 0, 6), name, False, Wf[:, :12].copy(), Ws[:, :12].copy(), bf, bs)
    with pytest.raises(ValueError, match="built without edge features"):
        gnnmp.cg_conv_ad(plain, g, xt, et)
    # nin != out under residual = True: the warning of cg_conv, and no residual in either direction (the layer test compares both)
    x4, e1, Wf4, Ws4, bf4, bs4, _ = R.layer_case((4, 1, 7), name)
    odd = make_layer((4, 1, 7), name, True, Wf4, Ws4, bf4, bs4)
    with pytest.warns(UserWarning, match="residual not applied"):
        y = gnnmp.cg_conv_ad(odd, g, dev(x4), dev(e1))
    with pytest.warns(UserWarning, match="residual not applied"):
        y_plain = gnnmp.cg_conv(odd, g, dev(x4), dev(e1))
    assert np.array_equal(bits(y.cpu().numpy()), bits(y_plain.cpu().numpy()))


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU 7: a small CGCNN step
# ------------------------------------------------------------------------------------------------------------------------------------
@gpu
def test_a_small_cgcnn_step():
    """radius_graph(pos) -> e = 8 Gaussian basis functions of the edge length (torch; a leaf that requires a gradient) -> two
    CGConv(((16, 8), 16), softplus, residual) -> global_pool_ad mean; 4 clouds of 48 points in the unit cube, loss = Σ pooled .* R: all
    parameter gradients, dx and de against the float64 chain on the edge list the device built.  The radius gives every cloud a mean
    degree of at least 4, no node more than 12 neighbours, and every node at least one."""
    import torch
    import gnnmp
    from gnnmp.backward import global_pool_ad
    pos, gi, x, layers, Rm = R.cgcnn_case()
    c = R.CGCNN
    n = len(pos)
    pd = dev(pos)
    g = gnnmp.radius_graph(pd, c["radius"], graph_indicator=dev(gi + 1))
    s, t = g.s.cpu().numpy() - 1, g.t.cpu().numpy() - 1
    assert np.array_equal(gi[s], gi[t]) and not (s == t).any()
    deg = np.bincount(t, minlength=n)
    per_cloud = deg.reshape(c["clouds"], c["pts"]).mean(axis=1)
    print(f"radius graph: {len(s)} edges, mean degree per cloud {per_cloud}, min {deg.min()}, max {deg.max()}")
    assert per_cloud.min() >= 4 and deg.max() <= 12 and deg.min() >= 1
    length = (pd[g.s - 1] - pd[g.t - 1]).norm(dim=1, keepdim=True)
    mu = torch.linspace(0.0, c["radius"], c["ein"], device="cuda")
    et = torch.exp(-((length - mu) / (c["radius"] / c["ein"])) ** 2).detach().contiguous().requires_grad_(True)
    ls = [make_layer((c["nin"], c["ein"], c["nin"]), "softplus", True, *w) for w in layers]
    for l in ls:
        for p in params(l):
            p.requires_grad_(True)
    xt = dev(x).requires_grad_(True)
    h1 = gnnmp.cg_conv_ad(ls[0], g, xt, et)
    h2 = gnnmp.cg_conv_ad(ls[1], g, h1, et)
    pooled = global_pool_ad(gnnmp.GlobalPool("mean"), g, h2)
    (pooled * dev(Rm)).sum().backward()
    torch.cuda.synchronize()
    e = et.detach().cpu().numpy()
    h2_ref, grads, dx_ref, de_ref = R.cgcnn_grad64(s, t, gi, x, e, layers, Rm)
    close(h2.detach().cpu().numpy(), h2_ref, "h2")
    for i, (l, ref) in enumerate(zip(ls, grads)):
        for p, k in zip(params(l), ("dWf", "dWs", "dbf", "dbs")):
            close(p.grad.cpu().numpy(), ref[k], f"{k} of layer {i + 1}")
    close(xt.grad.cpu().numpy(), dx_ref, "dx")
    close(et.grad.cpu().numpy(), de_ref, "de")
