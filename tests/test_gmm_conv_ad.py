"""gmm_conv_ad: GMMConv (MoNet) trained on the fused mixture-weight kernels (csrc/gmm.hip; include/gnnmp.h states the arithmetic).

Without a GPU: the three exports exist in header, SYMBOLS and library and take const plans and const host records; every refusal of the
header comes before any HIP call; empty sizes return OK; the float64 reference (tests/gmm_conv_ref.py) agrees with central finite
differences for all five activations and with oracle.more_layers.gmm_conv; the operands of every GPU case keep the float32 restatement
of the header's formulas within 2e-6 of float64 (w included) and, for relu, away from the kink.

On the GPU: y, z, dxk, dw of the two row exports within 1e-5 of float64, norm-wise and element-wise, at every lane width, tail, tile count
and register capacity, on a multigraph with self loops, repeated edges, a row without in-edges, a row without out-edges and a hub
destination and source of 600 edges; de within 1e-5, dmu / dsinv within the fp32 summation bound; every output element — `part` included —
written and nothing else, at any pointer alignment; the layer against the reference, the oracle and gnnmp.gmm_conv; equal bits of two calls;
each export recorded into a HIP graph without an eager call first; empty graphs; the refusals of gmm_conv_ad; a small MoNet step."""
import ctypes
import itertools
import os
import re
import subprocess
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_cases as A  # noqa: E402
import gmm_conv_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FWD, GRAD, WGRAD = "gnnmp_gmm_conv_f32", "gnnmp_gmm_conv_grad_f32", "gnnmp_gmm_weights_grad_f32"
gpu = pytest.mark.gpu
f32, f64 = np.float32, np.float64
RECORDS = {FWD: ("gnnmp_gmm_conv_t", "GmmConvJob", ("w", "xk", "bias", "y", "z", "act")),
           GRAD: ("gnnmp_gmm_conv_grad_t", "GmmConvGradJob", ("w", "xk", "dz", "dxk", "dw")),
           WGRAD: ("gnnmp_gmm_weights_grad_t", "GmmWeightsGradJob", ("e", "mu", "sinv", "w", "dw", "de", "dmu", "dsinv", "part"))}
PARAMS = {FWD: ["plan", "job", "K", "C", "stream"], GRAD: ["plan", "plan_t", "job", "K", "C", "stream"],
          WGRAD: ["job", "E", "ein", "K", "stream"]}


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
    for name in (FWD, GRAD, WGRAD):
        assert f"int {name}(" in header and header.index(f"int {name}(") < internal, name
        assert name in _lib.SYMBOLS and name in exported, name
        assert "} " + RECORDS[name][0] + ";" in header
    assert "GNNlib/src/layers/conv.jl:372-401" in header[:internal]
    assert "tests/test_gmm_conv_ad.py" in header[:header.index("#ifndef GNNMP_H")]           # the Conventions paragraph: what is tested
    assert int(re.search(r"#define GNNMP_GMM_PARTS (\d+)", header).group(1)) == _lib.GMM_PARTS == R.PARTS
    assert callable(gnnmp.gmm_conv_ad)


@pytest.mark.parametrize("export", [FWD, GRAD, WGRAD])
def test_the_exports_take_const_plans_and_const_host_records(export):
    """device pointers travel in const host records: the table of tests/abi_cases.py owes no case, this file carries the memory-contract
    and capture checks itself.  The ctypes records have the layout of the header's structs."""
    from gnnmp import _lib
    decls, _ = A.parse_header()
    assert export not in A.must_be_covered(decls, _lib.SYMBOLS)
    assert [p[0] for p in decls[export]] == PARAMS[export]
    for pname, is_ptr, is_const, _ in decls[export]:
        assert is_const or not is_ptr, pname
    struct, cls, want = RECORDS[export]
    header = open(os.path.join(ROOT, "include", "gnnmp.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} " + struct + ";", header).group(1)
    body = re.sub(r"/\*.*?\*/", " ", body, flags=re.S)
    fields, off, offsets = [], 0, []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        is_ptr = "*" in decl
        for nme in [n.strip().lstrip("*") for n in re.sub(r"^(const\s+)?(float|int)\s+", "", decl).split(",")]:
            size = 8 if is_ptr else 4
            off = (off + size - 1) // size * size
            fields.append(nme)
            offsets.append(off)
            off += size
    rec = getattr(_lib, cls)
    assert tuple(fields) == want == tuple(f for f, _ in rec._fields_)
    assert [getattr(rec, f).offset for f in want] == offsets
    assert ctypes.sizeof(rec) == (off + 7) // 8 * 8


P = lambda v: ctypes.c_void_p(0x1000 * v) if v else None      # never dereferenced: the call must refuse first  # noqa: E731


class _FakePlan(ctypes.Structure):
    """the head of csrc/common.h's gnnmp_graph {int64 n_src, n_dst, n_edges, n_total; ...}: all the refusals read of a plan"""
    _fields_ = [("n_src", ctypes.c_int64), ("n_dst", ctypes.c_int64), ("n_edges", ctypes.c_int64), ("n_total", ctypes.c_int64),
                ("tail", ctypes.c_char * 1024)]


def _fwd(lib, plan, job=True, w=1, xk=2, bias=3, y=4, z=5, act=0, K=3, C=4):
    from gnnmp import _lib
    j = _lib.GmmConvJob(P(w), P(xk), P(bias), P(y), P(z), act)
    return lib.gnnmp_gmm_conv_f32(plan, ctypes.byref(j) if job else None, K, C, None)


def _grad(lib, plan, plan_t, job=True, w=1, xk=2, dz=3, dxk=4, dw=5, K=3, C=4):
    from gnnmp import _lib
    j = _lib.GmmConvGradJob(P(w), P(xk), P(dz), P(dxk), P(dw))
    return lib.gnnmp_gmm_conv_grad_f32(plan, plan_t, ctypes.byref(j) if job else None, K, C, None)


def _wgrad(lib, job=True, e=1, mu=2, sinv=3, w=4, dw=5, de=6, dmu=7, dsinv=8, part=9, E=5, ein=3, K=3):
    from gnnmp import _lib
    j = _lib.GmmWeightsGradJob(P(e), P(mu), P(sinv), P(w), P(dw), P(de), P(dmu), P(dsinv), P(part))
    return lib.gnnmp_gmm_weights_grad_f32(ctypes.byref(j) if job else None, E, ein, K, None)


def test_argument_validation_needs_no_gpu():
    """every refusal of the header comes before the first HIP call: on a machine without a device, on pointers that are not memory"""
    from gnnmp import _lib
    lib = _lib.load()
    EINVAL, err = _lib.EINVAL, lib.gnnmp_last_error
    mk = lambda **kw: _FakePlan(**kw)      # noqa: E731
    sq, sq_t = mk(n_src=5, n_dst=5, n_edges=7, n_total=7), mk(n_src=5, n_dst=5, n_edges=7, n_total=7)
    pl, pt = ctypes.addressof(sq), ctypes.addressof(sq_t)
    rect = mk(n_src=9, n_dst=5, n_edges=7, n_total=7)
    tall, more = mk(n_src=6, n_dst=6, n_edges=7, n_total=7), mk(n_src=5, n_dst=5, n_edges=8, n_total=8)
    loops, loops_t = mk(n_src=5, n_dst=5, n_edges=7, n_total=12), mk(n_src=5, n_dst=5, n_edges=7, n_total=12)
    # the forward
    assert _fwd(lib, None) == EINVAL and b"null plan" in err()
    assert _fwd(lib, pl, job=False) == EINVAL and b"null job" in err()
    for name in ("w", "xk", "y"):
        assert _fwd(lib, pl, **{name: None}) == EINVAL and f"null {name}".encode() in err(), name
    for K in (0, -1, 17, 2 ** 40):
        assert _fwd(lib, pl, K=K) == EINVAL and b"bad K" in err(), K
    for K, C in ((3, 0), (3, -3), (1, (1 << 19) + 1), (3, 2 ** 40), (16, (1 << 16) + 1)):      # the last: K C > 2^20
        assert _fwd(lib, pl, K=K, C=C) == EINVAL and b"bad C" in err(), (K, C)
    for act in (-1, 5, 17):
        assert _fwd(lib, pl, act=act) == EINVAL and b"bad act" in err(), act
    assert _fwd(lib, ctypes.addressof(rect)) == EINVAL and b"not square" in err()
    assert _fwd(lib, ctypes.addressof(loops)) == EINVAL and b"self loops" in err()
    # the pullback of the row step
    assert _grad(lib, None, pt) == EINVAL and b"null plan" in err()
    assert _grad(lib, pl, None) == EINVAL and b"null plan_t" in err()
    assert _grad(lib, pl, pt, job=False) == EINVAL and b"null job" in err()
    assert _grad(lib, pl, pt, dxk=None, dw=None) == EINVAL and b"dxk and dw are both null" in err()
    assert _grad(lib, pl, pt, dz=None) == EINVAL and b"null dz" in err()
    assert _grad(lib, pl, pt, w=None) == EINVAL and b"dxk without w" in err()
    assert _grad(lib, pl, pt, xk=None) == EINVAL and b"dw without xk" in err()
    for K in (0, 17):
        assert _grad(lib, pl, pt, K=K) == EINVAL and b"bad K" in err(), K
    for C in (0, (1 << 19) + 1):
        assert _grad(lib, pl, pt, C=C) == EINVAL and b"bad C" in err(), C
    assert _grad(lib, ctypes.addressof(rect), pt) == EINVAL and b"not square" in err()
    assert _grad(lib, pl, ctypes.addressof(tall)) == EINVAL and b"the transposed plan has 6 rows, the plan 5" in err()
    assert _grad(lib, pl, ctypes.addressof(more)) == EINVAL and b"the transposed plan has 8 edges, the plan 7" in err()
    assert _grad(lib, ctypes.addressof(loops), ctypes.addressof(loops_t)) == EINVAL and b"self loops" in err()
    # the pullback of the mixture weights
    assert _wgrad(lib, job=False) == EINVAL and b"null job" in err()
    assert _wgrad(lib, E=-1) == EINVAL and b"negative E" in err()
    for ein in (0, -2, 65):
        assert _wgrad(lib, ein=ein) == EINVAL and b"bad ein" in err(), ein
    for K in (0, 17):
        assert _wgrad(lib, K=K) == EINVAL and b"bad K" in err(), K
    assert _wgrad(lib, de=None, dmu=None, dsinv=None) == EINVAL and b"all null" in err()
    assert _wgrad(lib, dmu=None) == EINVAL and b"come together" in err()
    assert _wgrad(lib, dsinv=None) == EINVAL and b"come together" in err()
    assert _wgrad(lib, part=None) == EINVAL and b"dmu without part" in err()
    for name in ("e", "mu", "sinv", "w", "dw"):
        assert _wgrad(lib, **{name: None}) == EINVAL and f"null {name}".encode() in err(), name


def test_empty_sizes_return_ok_without_a_device():
    """N = 0 (the row exports) and E = 0 (the weights' pullback) launch nothing — with and without the optional pointers"""
    from gnnmp import _lib
    lib = _lib.load()
    none = _FakePlan(n_src=0, n_dst=0, n_edges=0, n_total=0)
    pn = ctypes.addressof(none)
    assert _fwd(lib, pn) == _lib.OK
    assert _fwd(lib, pn, w=None, bias=None, z=None, act=4, K=16, C=1 << 16) == _lib.OK
    assert _grad(lib, pn, pn) == _lib.OK
    assert _grad(lib, pn, pn, dw=None, xk=None, w=None) == _lib.OK
    assert _grad(lib, pn, pn, dxk=None, w=None, K=1, C=1 << 19) == _lib.OK
    assert _wgrad(lib, E=0) == _lib.OK
    assert _wgrad(lib, E=0, e=None, w=None, dw=None, de=None, ein=64, K=16) == _lib.OK
    assert _wgrad(lib, E=0, dmu=None, dsinv=None, part=None) == _lib.OK


# ------------------------------------------------------------------------------------------------------------------------------------
# CPU: the references
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_bias", [False, True], ids=["no_bias", "bias"])
@pytest.mark.parametrize("name", R.ACTS)
@pytest.mark.parametrize("nin", [4, 5])
def test_reference_gradient_agrees_with_finite_differences(nin, name, with_bias):
    """central differences of the float64 composition: n = 30, E = 200, ein = 3, K = 3, out = 5, h = 1e-6, the residual asked for (nin = 4:
    not applied, nin != out; nin = 5: applied); relu's pre-activations are kept more than 100 h from the kink"""
    h = 1e-6
    s, t, n, x, e, mu, sinv, W, bias, dy = R.fd_case(nin, name, with_bias)
    ref = R.layer(s, t, n, x, e, mu, sinv, W, bias, name, True, dy, f64)
    z0, y0 = R.compose(s, t, n, x, e, mu, sinv, W, bias, name, True)
    assert np.abs(ref["z"] - z0).max() <= 1e-12 * max(np.abs(z0).max(), 1.0) and np.abs(ref["y"] - y0).max() <= 1e-12 * np.abs(y0).max()
    if name == "relu":
        assert np.abs(z0[z0 != 0]).min() > 100 * h
    loss = lambda: float((R.compose(s, t, n, x, e, mu, sinv, W, bias, name, True)[1] * dy).sum())      # noqa: E731
    operands = [(x, "dx"), (e, "de"), (mu, "dmu"), (sinv, "dsinv"), (W, "dW")] + ([(bias, "db")] if with_bias else [])
    for arr, what in operands:
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


LAYER_CASES = list(itertools.product(R.LAYER_SHAPES, R.LAYER_KS, R.ACTS, (False, True)))      # residual mode, K, act, bias


@pytest.mark.parametrize("mode,K,name,with_bias", LAYER_CASES)
def test_reference_forward_agrees_with_the_oracle(mode, K, name, with_bias):
    """the float64 reference's y against oracle.more_layers.gmm_conv (float32 numpy, 1-based indices) at 1e-5"""
    from oracle import more_layers as ML
    shape, residual = R.LAYER_SHAPES[mode]
    s, t = R.graph()
    x, e, mu, sinv, W, bias, _ = R.layer_case(shape, K, name)
    ref = R.layer_ref64(shape, K, name, residual, with_bias)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        y = ML.gmm_conv(s + 1, t + 1, R.N_NODES, x, e, mu, sinv, W, bias if with_bias else None, act=name, K=K, residual=residual)
    assert R.rel(y, ref["y"]) <= 1e-5 and np.abs(y - ref["y"]).max() <= 1e-5 * np.abs(ref["y"]).max()


@pytest.mark.parametrize("C,K", R.KERNEL_CASES)
def test_the_kernel_cases_are_well_conditioned(C, K):
    """THE CONDITION ON THE INPUTS, not a measurement: z, dxk, dw by the header's formulas in float32 are within 2e-6, norm-wise, of float64"""
    worst = R.kernel_condition(C, K)
    assert worst <= R.COND, f"the float32 restatement is {worst:.2e} from float64 (bound {R.COND:g})"


@pytest.mark.parametrize("E,ein,K", R.WGRAD_CASES)
def test_the_weights_cases_are_well_conditioned(E, ein, K):
    """de and w in float32 within 2e-6 of float64; the float32 restatement of dmu / dsinv uses at most a fifth of the summation bound"""
    de, w, summ = R.wgrad_condition(E, ein, K)
    assert de <= R.COND and w <= R.COND and summ <= 0.2, (de, w, summ)


@pytest.mark.parametrize("mode,K,name,with_bias", LAYER_CASES)
def test_the_layer_cases_are_well_conditioned(mode, K, name, with_bias):
    shape, residual = R.LAYER_SHAPES[mode]
    worst, summ, ratio = R.layer_condition(shape, K, name, residual, with_bias)
    assert worst <= R.COND, f"the float32 restatement is {worst:.2e} from float64 (bound {R.COND:g})"
    assert summ <= 0.2, f"the float32 restatement of dmu / dsinv uses {summ:.2f} of the summation bound"
    if name == "relu":
        assert ratio >= R.MARGIN, f"the smallest |z| is only {ratio:.1f} x the float32-float64 deviation of z"


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU helpers
# ------------------------------------------------------------------------------------------------------------------------------------
def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def close(got, ref, what, tol=1e-5):
    """the project's parity bar, norm-wise AND element-wise against the array scale"""
    got, ref = np.asarray(got, f64), np.asarray(ref, f64)
    assert got.shape == ref.shape, what
    assert np.all(np.isfinite(got)), f"{what}: non-finite"
    err, scale = np.linalg.norm(got - ref), np.linalg.norm(ref)
    worst = np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300) if ref.size else 0.0
    print(f"{what}: |got - ref| = {err:.3e}, |ref| = {scale:.3e}, ratio {err / max(scale, 1e-300):.2e}, element-wise {worst:.2e}")
    assert err <= tol * scale, f"{what}: {err:.3e} > {tol:g} * {scale:.3e}"
    assert worst <= tol, f"{what}: element-wise {worst:.2e} of the array scale"


def within_sum_bound(got, ref, mag, E, what):
    """|got − ref64| <= (d + 8) 2^-24 Σ_e |term_e|, element-wise; d = slice length + GNNMP_GMM_PARTS"""
    got, ref = np.asarray(got, f64), np.asarray(ref, f64)
    assert got.shape == ref.shape and np.all(np.isfinite(got)), what
    bound = R.sum_bound(E, mag)
    used = float((np.abs(got - ref) / np.maximum(bound, 1e-300)).max()) if got.size else 0.0
    print(f"{what}: uses {used:.3f} of the summation bound (depth {R.fold_depth(E)})")
    assert np.all(np.abs(got - ref) <= bound), f"{what}: {used:.2f} of the summation bound"


def ptr(v):
    return None if v is None else ctypes.c_void_p(v.data_ptr())


def call_fwd(lib, plan, w, xk, bias, y, z, act, K, C, stream=None):
    from gnnmp import _lib
    job = _lib.GmmConvJob(w, xk, bias, y, z, act)
    return lib.gnnmp_gmm_conv_f32(plan, ctypes.byref(job), K, C, stream)


def call_grad(lib, plan, plan_t, w, xk, dz, dxk, dw, K, C, stream=None):
    from gnnmp import _lib
    job = _lib.GmmConvGradJob(w, xk, dz, dxk, dw)
    return lib.gnnmp_gmm_conv_grad_f32(plan, plan_t, ctypes.byref(job), K, C, stream)


def call_wgrad(lib, e, mu, sinv, w, dw, de, dmu, dsinv, part, E, ein, K, stream=None):
    from gnnmp import _lib
    job = _lib.GmmWeightsGradJob(e, mu, sinv, w, dw, de, dmu, dsinv, part)
    return lib.gnnmp_gmm_weights_grad_f32(ctypes.byref(job), E, ein, K, stream)


@pytest.fixture(scope="module")
def lib():
    import torch
    assert torch.cuda.is_available()
    from gnnmp import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def graph(lib):
    """the multigraph of tests/cg_conv_ref.py as a GNNGraph with 0-based int64 indices; both plans DO split the hub rows (the row kernels
    here walk them whole)"""
    import gnnmp
    s, t = R.graph()
    R.assert_graph(s, t)
    g = gnnmp.GNNGraph(dev(s), dev(t), num_nodes=R.N_NODES, index_base=0)
    plan, plan_t = g.plan(False), g.plan_transposed(False)
    assert plan.n_long >= 1 and plan_t.n_long >= 1
    return g, s, t


def run_rows(lib, g, case, K, C, name="identity", want_z=True, want_dxk=True, want_dw=True):
    """(y, z | None, dxk | None, dw | None) of the two row exports as numpy arrays; outputs start as NaN"""
    import torch
    w, xk, bias, dz = [None if a is None else dev(a) for a in case]
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")      # noqa: E731
    n, E = xk.shape[0], w.shape[0]
    y, z = nan(n, C), nan(n, C) if want_z else None
    dxk, dw = nan(n, K * C) if want_dxk else None, nan(E, K) if want_dw else None
    plan, plan_t = g.plan(False).handle, g.plan_transposed(False).handle
    rc = call_fwd(lib, plan, ptr(w), ptr(xk), ptr(bias), ptr(y), ptr(z), R.ACT_CODE[name], K, C)
    assert rc == A.OK, lib.gnnmp_last_error()
    rc = call_grad(lib, plan, plan_t, ptr(w), ptr(xk), ptr(dz), ptr(dxk), ptr(dw), K, C)
    assert rc == A.OK, lib.gnnmp_last_error()
    torch.cuda.synchronize()
    return tuple(None if v is None else v.cpu().numpy() for v in (y, z, dxk, dw))


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU 1: the kernels against float64
# ------------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("C,K", R.KERNEL_CASES)
def test_row_kernels_against_float64(lib, graph, C, K):
    """C = 1, 3, 5, 33: 4-byte lanes (33: 64 lanes, 33 active); 2, 130: 8-byte lanes (130: a second tile with one active lane — the forward's
    second block column, the pullback's tile loop and its ordered update of dw); 4, 8, 64: 16-byte lanes.  K = 1, 2, 3, 4, 5, 16: the register
    capacities 1, 2, 3, 4, 8, 16, each at every lane width.  y, z, dxk, dw within 1e-5 of float64, norm-wise and element-wise; either output
    of the pullback has the same bits without the other; y = act(z) for the case's activation"""
    g, s, t = graph
    name = R.ACTS[(C + K) % 5]
    case = R.kernel_case(C, K)
    y, z, dxk, dw = run_rows(lib, g, case, K, C, name)
    z64, dxk64, dw64 = R.kernel_ref64(C, K)
    close(z, z64, "z")
    close(y, R.act(z64, name), "y")
    close(dxk, dxk64, "dxk")
    close(dw, dw64, "dw")
    indeg, outdeg = np.bincount(t, minlength=R.N_NODES), np.bincount(s, minlength=R.N_NODES)
    assert np.array_equal(z[indeg == 0], np.broadcast_to(case[2], (int((indeg == 0).sum()), C)))      # no in-edge: z = bias exactly
    assert not dxk[outdeg == 0].any()
    y2, z2, dxk2, dw2 = run_rows(lib, g, case, K, C, name, want_z=False, want_dw=False)
    assert z2 is None and dw2 is None and np.array_equal(bits(y2), bits(y)) and np.array_equal(bits(dxk2), bits(dxk))
    _, _, dxk3, dw3 = run_rows(lib, g, case, K, C, name, want_dxk=False)
    assert dxk3 is None and np.array_equal(bits(dw3), bits(dw))


def run_wgrad(lib, case, want_de=True, want_par=True):
    import torch
    e, mu, sinv, w, dw = [dev(a) for a in case]
    E, ein = e.shape
    K = mu.shape[0]
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")      # noqa: E731
    de = nan(E, ein) if want_de else None
    dmu, dsinv, part = (nan(K, ein), nan(K, ein), nan(R.PARTS, 2, K, ein)) if want_par else (None, None, None)
    rc = call_wgrad(lib, ptr(e), ptr(mu), ptr(sinv), ptr(w), ptr(dw), ptr(de), ptr(dmu), ptr(dsinv), ptr(part), E, ein, K)
    assert rc == A.OK, lib.gnnmp_last_error()
    torch.cuda.synchronize()
    return tuple(None if v is None else v.cpu().numpy() for v in (de, dmu, dsinv, part))


@gpu
@pytest.mark.parametrize("E,ein,K", R.WGRAD_CASES)
def test_weights_pullback_against_float64(lib, E, ein, K):
    """E = 1, 7 (most slices empty), 257 (two edges in the first slices, none in the last), 3 PARTS + 5 (every slice several edges, a ragged
    last one); de within 1e-5 norm-wise, dmu / dsinv within the summation bound, part fully written and its index-order sum is dmu / dsinv"""
    case = R.wgrad_case(E, ein, K)
    de, dmu, dsinv, part = run_wgrad(lib, case)
    de64, dmu64, dsinv64, mag_mu, mag_s = R.wgrad64(*case)
    close(de, de64, "de")
    within_sum_bound(dmu, dmu64, mag_mu, E, "dmu")
    within_sum_bound(dsinv, dsinv64, mag_s, E, "dsinv")
    assert np.all(np.isfinite(part))
    L = -(-E // R.PARTS)
    empty = np.arange(R.PARTS) * L >= E
    assert not part[empty].any()
    fold = np.zeros((2, K, ein), f32)
    for b in range(R.PARTS):
        fold = fold + part[b]
    assert np.array_equal(bits(fold[0]), bits(dmu)) and np.array_equal(bits(fold[1]), bits(dsinv))
    de2, _, _, _ = run_wgrad(lib, case, want_par=False)
    _, dmu2, dsinv2, _ = run_wgrad(lib, case, want_de=False)
    assert np.array_equal(bits(de2), bits(de)) and np.array_equal(bits(dmu2), bits(dmu)) and np.array_equal(bits(dsinv2), bits(dsinv))


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU 2: the layer
# ------------------------------------------------------------------------------------------------------------------------------------
def torch_act(name):
    import torch
    F = torch.nn.functional
    return {"identity": None, "relu": "relu", "softplus": F.softplus, "tanh": torch.tanh, "swish": F.silu}[name]


def make_layer(shape, K, name, residual, mu, sinv, W, bias):
    import gnnmp
    nin, ein, out = shape
    l = gnnmp.GMMConv(((nin, ein), out), name, K=K, bias=bias is not None, residual=residual)
    l.mu, l.sigma_inv, l.dense_x_weight = dev(mu), dev(sinv), dev(W)
    if bias is not None:
        l.bias = dev(bias)
    return l


def params(l):
    return [p for p in (l.mu, l.sigma_inv, l.dense_x_weight, l.bias) if p is not None]


def layer_grads(l, g, x, e, dy):
    """dict(y, dx, de, dmu, dsinv, dW, db) of gmm_conv_ad as numpy arrays (db None without bias)"""
    import torch
    import gnnmp
    xt, et = dev(x).requires_grad_(True), dev(e).requires_grad_(True)
    for p in params(l):
        p.requires_grad_(True)
        p.grad = None
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        y = gnnmp.gmm_conv_ad(l, g, xt, et)
    y.backward(dev(dy))
    torch.cuda.synchronize()
    np_ = lambda v: None if v is None else v.detach().cpu().numpy()      # noqa: E731
    grad = lambda p: None if p is None else np_(p.grad)      # noqa: E731
    return dict(y=np_(y), dx=grad(xt), de=grad(et), dmu=grad(l.mu), dsinv=grad(l.sigma_inv), dW=grad(l.dense_x_weight), db=grad(l.bias))


def check_layer(got, ref, E, with_bias):
    for k in ("y", "dx", "de", "dW"):
        close(got[k], ref[k], k)
    within_sum_bound(got["dmu"], ref["dmu"], ref["mag_mu"], E, "dmu")
    within_sum_bound(got["dsinv"], ref["dsinv"], ref["mag_s"], E, "dsinv")
    if with_bias:
        close(got["db"], ref["db"], "db")
    else:
        assert got["db"] is None


@gpu
@pytest.mark.parametrize("mode,K,name,with_bias", LAYER_CASES)
def test_layer_against_the_reference(graph, mode, K, name, with_bias):
    """gmm_conv_ad(...).backward(Δ): y within 1e-5 of the float64 reference, of the oracle and of gnnmp.gmm_conv; dx, de, d dense_x_weight,
    dbias within 1e-5, dmu and dsigma_inv within the summation bound; under no_grad no z is allocated and y has the same bits"""
    import torch
    import gnnmp
    from gnnmp import backward_gmm
    from oracle import more_layers as ML
    g, s, t = graph
    shape, residual = R.LAYER_SHAPES[mode]
    x, e, mu, sinv, W, bias, dy = R.layer_case(shape, K, name)
    if not with_bias:
        bias = None
    l = make_layer(shape, K, name, residual, mu, sinv, W, bias)
    got = layer_grads(l, g, x, e, dy)
    check_layer(got, R.layer_ref64(shape, K, name, residual, with_bias), len(e), with_bias)
    seen = []
    rows = backward_gmm.gmm_rows
    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        y_oracle = ML.gmm_conv(s + 1, t + 1, R.N_NODES, x, e, mu, sinv, W, bias, act=name, K=K, residual=residual)
        plain = make_layer(shape, K, torch_act(name), residual, mu, sinv, W, bias)
        y_plain = gnnmp.gmm_conv(plain, g, dev(x), dev(e))
        backward_gmm.gmm_rows = lambda *a: seen.append(a[-1]) or rows(*a)
        try:
            y_nograd = gnnmp.gmm_conv_ad(l, g, dev(x), dev(e))
        finally:
            backward_gmm.gmm_rows = rows
    close(got["y"], y_oracle, "y against the oracle")
    close(got["y"], y_plain.cpu().numpy(), "y against gnnmp.gmm_conv")
    assert seen == [False] and not y_nograd.requires_grad            # want_z = False: no z is allocated
    assert np.array_equal(bits(y_nograd.cpu().numpy()), bits(got["y"]))


@gpu
def test_what_needs_no_gradient_gets_none(graph):
    """requires_grad=False on a parameter or an input: its .grad stays None; the others are still within their bars"""
    import torch
    import gnnmp
    g, s, t = graph
    mode, K, name = "applied", 3, "softplus"
    shape, residual = R.LAYER_SHAPES[mode]
    x, e, mu, sinv, W, bias, dy = R.layer_case(shape, K, name)
    full = R.layer_ref64(shape, K, name, residual, True)
    names = ("dx", "de", "dmu", "dsinv", "dW", "db")
    for off in (("dx",), ("de",), ("dmu", "db"), ("de", "dmu", "dsinv"), ("dx", "dW"), ("dx", "de", "dmu", "dsinv", "dW"), names):
        l = make_layer(shape, K, name, residual, mu, sinv, W, bias)
        leaves = dict(dx=dev(x), de=dev(e), dmu=l.mu, dsinv=l.sigma_inv, dW=l.dense_x_weight, db=l.bias)
        for k in names:
            leaves[k].requires_grad_(k not in off)
        y = gnnmp.gmm_conv_ad(l, g, leaves["dx"], leaves["de"])
        if len(off) == len(names):
            assert not y.requires_grad
            continue
        y.backward(dev(dy))
        torch.cuda.synchronize()
        for k in names:
            if k in off:
                assert leaves[k].grad is None, (off, k)
            elif k in ("dmu", "dsinv"):
                within_sum_bound(leaves[k].grad.cpu().numpy(), full[k], full["mag_mu" if k == "dmu" else "mag_s"], len(e), f"{k} without {off}")
            else:
                close(leaves[k].grad.cpu().numpy(), full[k], f"{k} without {off}")


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU 3: the memory contract
# ------------------------------------------------------------------------------------------------------------------------------------
def contract_graph():
    s, t = R.graph()
    return A.Graph("gmm", s + 1, t + 1, R.N_NODES)


def rows_arrays(case, K, C, with_z=True, want_dxk=True, want_dw=True):
    w, xk, bias, dz = case
    arrs = [A.Arr("w", "in", w), A.Arr("xk", "in", xk), A.Arr("bias", "in", bias), A.Arr("dz", "in", dz), A.Arr("y", "out", shape=dz.shape)]
    arrs += [A.Arr("z", "out", shape=dz.shape)] if with_z else []
    arrs += [A.Arr("dxk", "out", shape=xk.shape)] if want_dxk else []
    return arrs + ([A.Arr("dw", "out", shape=w.shape)] if want_dw else [])


def rows_call(lib, slab, plan, plan_t, name, K, C, stream):
    p = lambda nm: slab.ptr(nm) if nm in slab.arrs else None      # noqa: E731
    rc = call_fwd(lib, plan, p("w"), p("xk"), p("bias"), p("y"), p("z"), R.ACT_CODE[name], K, C, stream)
    if rc != A.OK:
        return rc
    return call_grad(lib, plan, plan_t, p("w"), p("xk"), p("dz"), p("dxk"), p("dw"), K, C, stream)


def rows_want(slab, C, K, name, seed=0):
    z, dxk, dw = R.kernel_ref64(C, K, seed)
    want = {"y": A.E(R.act(z, name)), "z": A.E(z), "dxk": A.E(dxk), "dw": A.E(dw)}
    return {k: v for k, v in want.items() if k in slab.arrs}


@gpu
@pytest.mark.parametrize("C,K", [(8, 3), (2, 16), (130, 2)])
def test_memory_contract_of_the_row_exports(lib, C, K):
    """every element of y, z, dxk, dw written, no store before or after an array or into an input, with each array in turn shifted to 16-,
    8- and 4-byte alignment (C = 8: 16-byte lanes narrow to 8 and 4; C = 2, 130: 8-byte lanes narrow to 4), on a side stream — the hub rows
    included; once without z, once with dxk only, once with dw only"""
    import torch
    side = torch.cuda.Stream()
    sp = ctypes.c_void_p(side.cuda_stream)
    plans = A.Plans(lib)
    g = contract_graph()
    case = R.kernel_case(C, K)
    try:
        plan, plan_t = plans.get(A.Pl(g)), plans.get(A.Pl(g, T=True))
        names = [a.name for a in rows_arrays(case, K, C)]
        runs = [({}, {})] + [({nm: A.SHIFTS[a]}, {}) for nm in names for a in ("a16", "a8", "a4")]
        runs += [({}, dict(with_z=False)), ({"xk": 4}, dict(want_dw=False)), ({"dz": 8}, dict(want_dxk=False))]
        for k, (shifts, opts) in enumerate(runs):
            name = R.ACTS[k % 5]
            slab = A.Slab(rows_arrays(case, K, C, **opts), "cuda", shifts)
            torch.cuda.synchronize()
            rc = rows_call(lib, slab, plan, plan_t, name, K, C, sp)
            torch.cuda.synchronize()
            assert rc == A.OK, (shifts, lib.gnnmp_last_error())
            problems = slab.check(rows_want(slab, C, K, name))
            assert not problems, (name, shifts, opts, problems)
    finally:
        plans.close()


def wgrad_arrays(case, want_de=True, want_par=True):
    e, mu, sinv, w, dw = case
    arrs = [A.Arr(nm, "in", a) for nm, a in zip(("e", "mu", "sinv", "w", "dw"), case)]
    arrs += [A.Arr("de", "out", shape=e.shape)] if want_de else []
    if want_par:
        arrs += [A.Arr("dmu", "out", shape=mu.shape), A.Arr("dsinv", "out", shape=mu.shape), A.Arr("part", "out", shape=(R.PARTS, 2) + mu.shape)]
    return arrs


def wgrad_call(lib, slab, case, stream):
    p = lambda nm: slab.ptr(nm) if nm in slab.arrs else None      # noqa: E731
    E, ein = case[0].shape
    return call_wgrad(lib, p("e"), p("mu"), p("sinv"), p("w"), p("dw"), p("de"), p("dmu"), p("dsinv"), p("part"), E, ein, case[1].shape[0], stream)


def wgrad_want(slab, case):
    de64, dmu64, dsinv64, mag_mu, mag_s = R.wgrad64(*case)
    E = len(case[0])

    def bounded(ref, mag):
        return lambda got: None if np.all(np.abs(got.astype(f64) - ref) <= R.sum_bound(E, mag)) else "outside the summation bound"
    want = {"de": A.E(de64), "dmu": A.E(pred=bounded(dmu64, mag_mu)), "dsinv": A.E(pred=bounded(dsinv64, mag_s)),
            "part": A.E(pred=lambda got: None if np.all(np.isfinite(got)) else "non-finite partials")}      # every element written: the slab's own check
    return {k: v for k, v in want.items() if k in slab.arrs}


@gpu
@pytest.mark.parametrize("E,ein,K", [(R.PARTS * 3 + 5, 3, 3), (7, 5, 3), (257, 1, 16)])
def test_memory_contract_of_the_weights_pullback(lib, E, ein, K):
    """every element of de, dmu, dsinv and of part written — the slices without edges included — and nothing beyond, at several pointer
    alignments, with and without de and the parameter gradients"""
    import torch
    side = torch.cuda.Stream()
    sp = ctypes.c_void_p(side.cuda_stream)
    case = R.wgrad_case(E, ein, K)
    names = [a.name for a in wgrad_arrays(case)]
    runs = [({}, {})] + [({nm: A.SHIFTS[a]}, {}) for nm in names for a in ("a8", "a4")]
    runs += [({"e": 4}, dict(want_de=False)), ({"dw": 4}, dict(want_par=False))]
    for shifts, opts in runs:
        slab = A.Slab(wgrad_arrays(case, **opts), "cuda", shifts)
        torch.cuda.synchronize()
        rc = wgrad_call(lib, slab, case, sp)
        torch.cuda.synchronize()
        assert rc == A.OK, (shifts, lib.gnnmp_last_error())
        problems = slab.check(wgrad_want(slab, case))
        assert not problems, (shifts, opts, problems)


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU 4 and 5: capture, determinism, empty graphs
# ------------------------------------------------------------------------------------------------------------------------------------
def _capture_and_replay(lib, slab, call, reloads, wants):
    """record `call` (capture_error_mode = thread_local: a host wait or an allocation would be an error; the outputs still hold poison
    after the capture), replay it with each set of new values in the same buffers, then compare each replay bit for bit with an eager call"""
    import torch
    side = torch.cuda.Stream()
    sp = ctypes.c_void_p(side.cuda_stream)
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        graph.capture_begin(capture_error_mode="thread_local")
        try:
            rc = call(sp)
        finally:
            graph.capture_end()
    torch.cuda.synchronize()
    assert rc == A.OK, lib.gnnmp_last_error()
    assert not slab.check({}, untouched=True), "work ran while the call was being recorded"
    replayed = []
    for inputs, want in zip(reloads, wants):
        slab.reload(inputs)
        graph.replay()
        torch.cuda.synchronize()
        assert not slab.check(want)
        replayed.append(slab.outputs())
    for inputs, rep in zip(reloads, replayed):
        slab.reload(inputs)
        torch.cuda.synchronize()
        assert call(sp) == A.OK, lib.gnnmp_last_error()
        torch.cuda.synchronize()
        eager = slab.outputs()
        assert all(np.array_equal(eager[k], rep[k]) for k in eager)
    del graph


@gpu
def test_the_row_exports_record_into_a_hip_graph_without_an_eager_call(lib):
    C, K, name = 8, 3, "swish"
    g = contract_graph()
    cases = [R.kernel_case(C, K, seed=sd) for sd in (100, 101)]
    assert not np.array_equal(cases[0][0], cases[1][0])
    plans = A.Plans(lib)
    try:
        plan, plan_t = plans.get(A.Pl(g)), plans.get(A.Pl(g, T=True))
        for which in ("forward", "pullback"):
            keep = ("w", "xk", "bias", "y", "z") if which == "forward" else ("w", "xk", "dz", "dxk", "dw")
            slab = A.Slab([a for a in rows_arrays(cases[0], K, C) if a.name in keep])
            p = lambda nm: slab.ptr(nm) if nm in slab.arrs else None      # noqa: E731
            if which == "forward":
                call = lambda sp: call_fwd(lib, plan, p("w"), p("xk"), p("bias"), p("y"), p("z"), R.ACT_CODE[name], K, C, sp)      # noqa: E731
            else:
                call = lambda sp: call_grad(lib, plan, plan_t, p("w"), p("xk"), p("dz"), p("dxk"), p("dw"), K, C, sp)      # noqa: E731
            reloads = [{k: v for k, v in zip(("w", "xk", "bias", "dz"), case) if k in slab.arrs} for case in cases]
            wants = [rows_want(slab, C, K, name, seed=sd) for sd in (100, 101)]
            _capture_and_replay(lib, slab, call, reloads, wants)
    finally:
        plans.close()


@gpu
def test_the_weights_pullback_records_into_a_hip_graph_without_an_eager_call(lib):
    E, ein, K = R.PARTS * 3 + 5, 3, 3
    cases = [R.wgrad_case(E, ein, K, seed=sd) for sd in (100, 101)]
    slab = A.Slab(wgrad_arrays(cases[0]))
    reloads = [dict(zip(("e", "mu", "sinv", "w", "dw"), case)) for case in cases]
    _capture_and_replay(lib, slab, lambda sp: wgrad_call(lib, slab, cases[0], sp), reloads, [wgrad_want(slab, case) for case in cases])


@gpu
def test_two_calls_give_equal_bits(lib, graph):
    g, _, _ = graph
    for C, K in ((64, 3), (130, 2), (5, 16)):
        case = R.kernel_case(C, K)
        first, again = run_rows(lib, g, case, K, C, "tanh"), run_rows(lib, g, case, K, C, "tanh")
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(first, again)), (C, K)
    case = R.wgrad_case(R.PARTS * 3 + 5, 3, 3)
    first, again = run_wgrad(lib, case), run_wgrad(lib, case)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(first, again))
    shape, residual = R.LAYER_SHAPES["applied"]
    x, e, mu, sinv, W, bias, dy = R.layer_case(shape, 3, "swish")
    l = make_layer(shape, 3, "swish", residual, mu, sinv, W, bias)
    first, again = layer_grads(l, g, x, e, dy), layer_grads(l, g, x, e, dy)
    for k in R.WHAT:
        assert np.array_equal(bits(first[k]), bits(again[k])), k


@gpu
def test_empty_graphs(lib):
    """N = 0 launches nothing (the plan's head says so); a graph without edges gives y = σ(bias), dx = Δ under the residual, and zero
    gradients to e, mu and sigma_inv"""
    import torch
    import gnnmp
    none = _FakePlan(n_src=0, n_dst=0, n_edges=0, n_total=0)
    assert _fwd(lib, ctypes.addressof(none)) == A.OK and _grad(lib, ctypes.addressof(none), ctypes.addressof(none)) == A.OK
    assert _wgrad(lib, E=0) == A.OK
    n = 9
    nothing = np.zeros(0, np.int64)
    g = gnnmp.GNNGraph(dev(nothing), dev(nothing), num_nodes=n, index_base=0)
    shape, K, name = (6, 3, 6), 3, "softplus"
    x, _, mu, sinv, W, bias, dy = R.layer_case(shape, K, name)
    x, dy = x[:n], dy[:n]
    l = make_layer(shape, K, name, True, mu, sinv, W, bias)
    got = layer_grads(l, g, x, np.zeros((0, 3), f32), dy)
    sig_b = R.act(bias.astype(f64), name)
    close(got["y"], sig_b[None, :] + x, "y = σ(bias) + x")
    assert got["de"].shape == (0, 3) and not got["dmu"].any() and not got["dsinv"].any() and not got["dW"].any()
    assert np.array_equal(bits(got["dx"]), bits(dy))
    close(got["db"], (dy.astype(f64) * R.dact(np.broadcast_to(bias.astype(f64), dy.shape), name)).sum(axis=0), "db")
    with torch.no_grad():
        plain = gnnmp.gmm_conv_ad(make_layer(shape, K, name, False, mu, sinv, W, None), g, dev(x), dev(np.zeros((0, 3), f32)))
    close(plain.cpu().numpy(), np.full((n, 6), np.log(2.0)), "y = softplus(0) without bias")


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU 6: what gmm_conv_ad refuses
# ------------------------------------------------------------------------------------------------------------------------------------
@gpu
def test_gmm_conv_ad_refuses_by_name(graph):
    import torch
    import gnnmp
    g, _, _ = graph
    shape, K, name = (6, 3, 6), 3, "softplus"
    x, e, mu, sinv, W, bias, _ = R.layer_case(shape, K, name)
    l = make_layer(shape, K, name, False, mu, sinv, W, bias)
    xt, et = dev(x), dev(e)
    with pytest.raises(NotImplementedError, match="bipartite"):
        gnnmp.gmm_conv_ad(l, g, (xt, xt), et)
    with pytest.raises(ValueError, match="e has 2 pseudo-coordinates, the layer was built for 3"):
        gnnmp.gmm_conv_ad(l, g, xt, et[:, :2].contiguous())
    with pytest.raises(ValueError, match="x has 5 features, the layer was built for 6"):
        gnnmp.gmm_conv_ad(l, g, xt[:, :5].contiguous(), et)
    with pytest.raises(ValueError, match="callable"):
        gnnmp.gmm_conv_ad(make_layer(shape, K, torch.tanh, False, mu, sinv, W, bias), g, xt, et)
    with pytest.raises(ValueError, match="not in the gnnmp_act set"):
        gnnmp.gmm_conv_ad(make_layer(shape, K, "gelu", False, mu, sinv, W, bias), g, xt, et)
    big = make_layer(shape, K, name, False, mu, sinv, W, bias)
    big.K = 17
    with pytest.raises(ValueError, match="K > 16"):
        gnnmp.gmm_conv_ad(big, g, xt, et)
    x4, e2, mu2, sinv2, W4, b7, _ = R.layer_case((4, 2, 7), K, name)
    odd = make_layer((4, 2, 7), K, name, True, mu2, sinv2, W4, b7)
    with pytest.warns(UserWarning, match="Residual not applied"):
        gnnmp.gmm_conv_ad(odd, g, dev(x4), dev(e2))


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU 7: a small MoNet step
# ------------------------------------------------------------------------------------------------------------------------------------
@gpu
def test_a_small_monet_step():
    """knn_graph(pos, k = 6) on 4 clouds of 64 points -> e = the relative positions (pseudo-coordinates, ein = 3) -> GMMConv((8, 3) => 16,
    relu, K = 3) -> GMMConv((16, 3) => 16, K = 3, residual) -> global mean pool; loss = Σ pooled²: every gradient is finite, and one plain
    SGD step lowers the loss"""
    import torch
    import gnnmp
    from gnnmp.backward import global_pool_ad
    c = R.MONET
    rng = np.random.default_rng(c["seed"])
    n = c["clouds"] * c["pts"]
    pos = dev(rng.uniform(0, 1, (n, 3)).astype(f32))
    gi = dev(np.repeat(np.arange(1, c["clouds"] + 1), c["pts"]))
    g = gnnmp.knn_graph(pos, c["k"], graph_indicator=gi)
    assert g.num_edges == n * c["k"]
    e = (pos[g.s - 1] - pos[g.t - 1]).contiguous().requires_grad_(True)
    x = dev(rng.standard_normal((n, c["nin"])).astype(f32)).requires_grad_(True)
    layers = [gnnmp.GMMConv(((c["nin"], 3), c["hid"]), "relu", K=c["K"], seed=11),
              gnnmp.GMMConv(((c["hid"], 3), c["hid"]), None, K=c["K"], residual=True, seed=21)]
    leaves = [p for l in layers for p in params(l)]
    for p in leaves:
        p.requires_grad_(True)

    def loss():
        h = gnnmp.gmm_conv_ad(layers[0], g, x, e)
        h = gnnmp.gmm_conv_ad(layers[1], g, h, e)
        return (global_pool_ad(gnnmp.GlobalPool("mean"), g, h) ** 2).sum()
    before = loss()
    before.backward()
    before = before.detach()
    torch.cuda.synchronize()
    for v in leaves + [x, e]:
        assert v.grad is not None and bool(torch.isfinite(v.grad).all()) and bool((v.grad != 0).any())
    gsq = sum(float((p.grad.double() ** 2).sum()) for p in leaves)
    lr = 0.05 * float(before) / gsq          # a step that would cut a linear loss by 5 %
    with torch.no_grad():
        for p in leaves:
            p -= lr * p.grad
        after = loss()
    print(f"loss {float(before):.6f} -> {float(after):.6f} (lr {lr:.3e})")
    assert float(after) < float(before)
