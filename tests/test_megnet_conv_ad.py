"""megnet_conv_ad: MEGNetConv trained on the fused edge-update kernels (csrc/megnet.hip; include/gnnmp.h states the arithmetic), and the
pullback of aggregate_neighbors.

Without a GPU: the three exports exist in header, SYMBOLS and library and take const plans and const host records whose ctypes mirrors
have the header's layout; every refusal of the header comes before any HIP call; N = 0 returns OK; the float64 reference
(tests/megnet_conv_ref.py) agrees with central finite differences for all five first-layer activations and all four folds, with and
without biases, with x̄, ē or both in the loss, and with oracle.more_layers.megnet_conv; the operands of every GPU case keep the float32
restatement of the header's formulas within 2e-6 of float64, relu's pre-activations 1e-3 from 0 and max / min's winners 1e-3 ahead.

On the GPU: every export within 1e-5 of float64, norm-wise and element-wise, at every lane width, tail and tile count, on a multigraph of
40 nodes with self loops, a repeated edge carrying an exact tie, a node without in-edges, one without out-edges and a hub of 600 edges
in and 600 out; the optional outputs do not change the others' bits; every output element written and nothing else, at any pointer
alignment; equal bits of two calls; each export recorded into a HIP graph without an eager call first; empty graphs; megnet_conv_ad
against the reference, the oracle and gnnmp.megnet_conv; every gradient (dx, de at 1e-5; weights and biases inside the fp32 summation
bound γ_n Σ|terms|, n = E, the longest fold on the path: tests/megnet_conv_ref.py, grad); pruning, refusals, aggregate_neighbors_ad; a MEGNet step."""
import ctypes
import itertools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_cases as A  # noqa: E402
import megnet_conv_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EDGE, GRAD, AGG = "gnnmp_megnet_edge_f32", "gnnmp_megnet_edge_grad_f32", "gnnmp_aggregate_grad_f32"
gpu = pytest.mark.gpu
f32, f64 = np.float32, np.float64
RECORDS = {EDGE: ("gnnmp_megnet_edge_t", "MegnetEdgeJob", ("P", "Q", "F", "a0", "z0", "act")),
           GRAD: ("gnnmp_megnet_edge_grad_t", "MegnetEdgeGradJob", ("da0", "z", "dz0", "dP", "dQ", "act")),
           AGG: ("gnnmp_aggregate_grad_t", "AggregateGradJob", ("dy", "m", "y", "acc", "dm"))}
PARAMS = {EDGE: ["plan", "job", "hid", "stream"], GRAD: ["plan", "plan_t", "job", "hid", "stream"], AGG: ["plan", "job", "aggr", "D", "stream"]}


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
    for name in (EDGE, GRAD, AGG):
        assert f"int {name}(" in header and header.index(f"int {name}(") < internal, name
        assert name in _lib.SYMBOLS and name in exported, name
        assert "} " + RECORDS[name][0] + ";" in header
    assert "GNNlib/src/layers/conv.jl:356-368" in header[:internal] and "msgpass.jl:145-149" in header[:internal]
    assert "tests/test_megnet_conv_ad.py" in header[:header.index("#ifndef GNNMP_H")]           # the Conventions paragraph: what is tested
    assert callable(gnnmp.megnet_conv_ad) and callable(gnnmp.aggregate_neighbors_ad)


@pytest.mark.parametrize("export", [EDGE, GRAD, AGG])
def test_the_exports_take_const_plans_and_const_host_records(export):
    """device pointers travel in const host records: the table of tests/abi_cases.py owes no case, this file carries the memory-contract
    and capture checks itself.  The ctypes records have the layout of the header's structs: names, offsets, size."""
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


P_ = lambda v: ctypes.c_void_p(0x1000 * v) if v else None      # never dereferenced: the call must refuse first  # noqa: E731


class _FakePlan(ctypes.Structure):
    """the head of csrc/common.h's gnnmp_graph {int64 n_src, n_dst, n_edges, n_total; ...}: all the refusals read of a plan"""
    _fields_ = [("n_src", ctypes.c_int64), ("n_dst", ctypes.c_int64), ("n_edges", ctypes.c_int64), ("n_total", ctypes.c_int64),
                ("tail", ctypes.c_char * 1024)]


def _edge(lib, plan, job=True, P=1, Q=2, F=3, a0=4, z0=5, act=0, hid=4):
    from gnnmp import _lib
    j = _lib.MegnetEdgeJob(P_(P), P_(Q), P_(F), P_(a0), P_(z0), act)
    return lib.gnnmp_megnet_edge_f32(plan, ctypes.byref(j) if job else None, hid, None)


def _grad(lib, plan, plan_t, job=True, da0=1, z=2, dz0=3, dP=4, dQ=5, act=1, hid=4):
    from gnnmp import _lib
    j = _lib.MegnetEdgeGradJob(P_(da0), P_(z), P_(dz0), P_(dP), P_(dQ), act)
    return lib.gnnmp_megnet_edge_grad_f32(plan, plan_t, ctypes.byref(j) if job else None, hid, None)


def _agg(lib, plan, job=True, dy=1, m=2, y=3, acc=4, dm=5, aggr=2, D=4):
    from gnnmp import _lib
    j = _lib.AggregateGradJob(P_(dy), P_(m), P_(y), P_(acc), P_(dm))
    return lib.gnnmp_aggregate_grad_f32(plan, ctypes.byref(j) if job else None, aggr, D, None)


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
    bad_widths = (0, -1, (1 << 19) + 1, 2 ** 40)
    # the edge step
    assert _edge(lib, None) == EINVAL and b"null plan" in err()
    assert _edge(lib, pl, job=False) == EINVAL and b"null job" in err()
    for name in ("P", "Q", "a0"):
        assert _edge(lib, pl, **{name: None}) == EINVAL and f"null {name}".encode() in err(), name
    for hid in bad_widths:
        assert _edge(lib, pl, hid=hid) == EINVAL and b"bad hid" in err(), hid
    for act in (-1, 5, 17):
        assert _edge(lib, pl, act=act) == EINVAL and b"bad act" in err(), act
    assert _edge(lib, ctypes.addressof(rect)) == EINVAL and b"not square" in err()
    assert _edge(lib, ctypes.addressof(loops)) == EINVAL and b"self loops" in err()
    # its pullback
    assert _grad(lib, None, pt) == EINVAL and b"null plan" in err()
    assert _grad(lib, pl, None) == EINVAL and b"null plan_t" in err()
    assert _grad(lib, pl, pt, job=False) == EINVAL and b"null job" in err()
    assert _grad(lib, pl, pt, dz0=None, dP=None, dQ=None) == EINVAL and b"all null" in err()
    assert _grad(lib, pl, pt, dP=None) == EINVAL and b"come together" in err()
    assert _grad(lib, pl, pt, dQ=None) == EINVAL and b"come together" in err()
    assert _grad(lib, pl, pt, da0=None) == EINVAL and b"null da0" in err()
    for act in (1, 2, 3, 4):
        assert _grad(lib, pl, pt, z=None, act=act) == EINVAL and b"null z" in err(), act
    for hid in bad_widths:
        assert _grad(lib, pl, pt, hid=hid) == EINVAL and b"bad hid" in err(), hid
    for act in (-1, 5):
        assert _grad(lib, pl, pt, act=act) == EINVAL and b"bad act" in err(), act
    assert _grad(lib, ctypes.addressof(rect), pt) == EINVAL and b"not square" in err()
    assert _grad(lib, pl, ctypes.addressof(tall)) == EINVAL and b"the transposed plan has 6 rows, the plan 5" in err()
    assert _grad(lib, pl, ctypes.addressof(more)) == EINVAL and b"the transposed plan has 8 edges, the plan 7" in err()
    assert _grad(lib, ctypes.addressof(loops), ctypes.addressof(loops_t)) == EINVAL and b"self loops" in err()
    # the pullback of aggregate_neighbors
    assert _agg(lib, None) == EINVAL and b"null plan" in err()
    assert _agg(lib, pl, job=False) == EINVAL and b"null job" in err()
    for aggr in (-1, 4, 9):
        assert _agg(lib, pl, aggr=aggr) == EINVAL and b"bad aggr" in err(), aggr
    for D in bad_widths:
        assert _agg(lib, pl, D=D) == EINVAL and b"bad D" in err(), D
    for aggr in (0, 1, 2, 3):
        assert _agg(lib, pl, dy=None, aggr=aggr) == EINVAL and b"null dy" in err(), aggr
        assert _agg(lib, pl, dm=None, aggr=aggr) == EINVAL and b"null dm" in err(), aggr
    for aggr in (2, 3):
        assert _agg(lib, pl, m=None, aggr=aggr) == EINVAL and b"null m" in err(), aggr
        assert _agg(lib, pl, y=None, aggr=aggr) == EINVAL and b"null y" in err(), aggr
    assert _agg(lib, ctypes.addressof(loops)) == EINVAL and b"self loops" in err()


def test_empty_sizes_return_ok_without_a_device():
    """N = 0 launches nothing — with and without the optional pointers; gnnmp_aggregate_grad_f32 takes a plan that is not square"""
    from gnnmp import _lib
    lib = _lib.load()
    none = _FakePlan(n_src=0, n_dst=0, n_edges=0, n_total=0)
    pn = ctypes.addressof(none)
    assert _edge(lib, pn) == _lib.OK
    assert _edge(lib, pn, F=None, z0=None, a0=None, act=4, hid=1 << 19) == _lib.OK
    assert _grad(lib, pn, pn) == _lib.OK
    assert _grad(lib, pn, None, dP=None, dQ=None) == _lib.OK
    assert _grad(lib, pn, pn, dz0=None, z=None, act=0, da0=None) == _lib.OK
    for aggr in (0, 1, 2, 3):
        assert _agg(lib, pn, aggr=aggr) == _lib.OK
    assert _agg(lib, pn, m=None, y=None, acc=None, aggr=0, D=1 << 19) == _lib.OK
    no_dst = _FakePlan(n_src=9, n_dst=0, n_edges=0, n_total=0)
    assert _agg(lib, ctypes.addressof(no_dst)) == _lib.OK


# ------------------------------------------------------------------------------------------------------------------------------------
# CPU: the references
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("bias", [False, True], ids=["no_bias", "bias"])
@pytest.mark.parametrize("aggr", R.AGGRS)
@pytest.mark.parametrize("name", R.ACTS)
def test_reference_gradient_agrees_with_finite_differences(name, aggr, bias, mode):
    """central differences of the float64 layer, h = 1e-6, loss = Σ x̄ ⊙ Rx (mode x), Σ ē ⊙ Re (mode e) or both: dx, de and every weight
    and bias of ϕe and ϕv; relu's pre-activations and max / min's leads are kept more than 100 h from their kinks (R.fd_case)"""
    h = 1e-6
    s, t, n, x, e, phi_e, phi_v, dxb, deb = R.fd_case(name, aggr, bias, h)
    dxb, deb = (dxb if mode in ("x", "both") else None), (deb if mode in ("e", "both") else None)
    ref = R.grad(s, t, n, x, e, phi_e, phi_v, aggr, dxb, deb)

    def loss():
        xb, eb = R.forward(s, t, n, x, e, phi_e, phi_v, aggr)
        return (0.0 if dxb is None else float((xb * dxb).sum())) + (0.0 if deb is None else float((eb * deb).sum()))
    operands = [(x, ref["dx"], "dx"), (e, ref["de"], "de")]
    for cname, chain in (("phi_e", phi_e), ("phi_v", phi_v)):
        for q, (W, b, _) in enumerate(chain):
            got = ref[cname][q] if ref[cname][q] is not None else (np.zeros_like(W), None if b is None else np.zeros_like(b))
            operands.append((W, got[0], f"{cname}[{q}].W"))
            if b is not None:
                operands.append((b, got[1], f"{cname}[{q}].b"))
    for arr, g, what in operands:
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


LAYER_CASES = list(itertools.product(R.LAYER_SHAPES, R.AGGRS))


def _oracle(shape, aggr):
    from oracle import more_layers as ML
    s, t, _ = R.graph()
    x, e, phi_e, phi_v, _, _ = R.layer_case(shape, aggr)
    with np.errstate(invalid="ignore"):      # max / min: the -Inf / +Inf row of the node without in-edges goes through ϕv
        return ML.megnet_conv(s + 1, t + 1, R.N_NODES, x, e, phi_e, phi_v, aggr=aggr)


@pytest.mark.parametrize("shape,aggr", LAYER_CASES)
def test_reference_forward_agrees_with_the_oracle(shape, aggr):
    """the float64 reference's x̄ and ē against oracle.more_layers.megnet_conv (float32 numpy, 1-based indices) at 1e-5"""
    ref = R.layer_ref64(shape, aggr, "both")
    xb, eb = _oracle(shape, aggr)
    for got, want in ((xb, ref["xb"]), (eb, ref["eb"])):
        assert R.rel(got, want) <= 1e-5
        got, want, _ = R.split_nonfinite(got, want)
        assert np.abs(got - want).max() <= 1e-5 * np.abs(want).max()


@pytest.mark.parametrize("with_F", [True, False], ids=["F", "no_F"])
@pytest.mark.parametrize("name", R.ACTS)
@pytest.mark.parametrize("hid", R.WIDTHS)
def test_the_edge_cases_are_well_conditioned(hid, name, with_F):
    """THE CONDITION ON THE INPUTS, not a measurement: a0, z0, dz0, dP, dQ by the header's formulas in float32 are within 2e-6, norm-wise,
    of float64, and for relu no pre-activation is closer than 1e-3 to 0"""
    worst, kink = R.edge_condition(hid, name, with_F)
    assert worst <= R.COND, f"the float32 restatement is {worst:.2e} from float64 (bound {R.COND:g})"
    assert name != "relu" or kink >= R.KINK, kink


@pytest.mark.parametrize("with_acc", [True, False], ids=["acc", "no_acc"])
@pytest.mark.parametrize("aggr", R.AGGRS)
@pytest.mark.parametrize("D", R.WIDTHS)
def test_the_aggregate_cases_are_well_conditioned(D, aggr, with_acc):
    """dm in float32 within 2e-6 of float64; under max / min every winner leads its runner-up by 1e-3 — but for the deliberate tie"""
    worst, lead = R.aggr_condition(D, aggr, with_acc)
    assert worst <= R.COND and lead >= R.KINK, (worst, lead)
    if aggr in ("max", "min"):
        s, t, (k1, k2) = R.graph()
        dy, m, y, acc = R.aggr_case(D, aggr)
        assert np.array_equal(m[k1], m[k2]) and m[k1, 0] == y[t[k1], 0]      # the tie, and in channel 0 the tie wins


@pytest.mark.parametrize("shape,aggr", LAYER_CASES)
def test_the_layer_cases_are_well_conditioned(shape, aggr):
    worst, kink, lead = R.layer_condition(shape, aggr)
    assert worst <= R.COND, f"the float32 restatement is {worst:.2e} from float64 (bound {R.COND:g})"
    assert kink >= R.KINK, f"a relu pre-activation is {kink:.2e} from 0"
    assert lead >= R.KINK, f"a winner leads by only {lead:.2e}"
    s, t, (k1, k2) = R.graph()
    x, e, *_ = R.layer_case(shape, aggr)
    assert np.array_equal(e[k1], e[k2])


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU helpers
# ------------------------------------------------------------------------------------------------------------------------------------
def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def close(got, ref, what, tol=1e-5):
    """the project's parity bar, norm-wise AND element-wise against the array scale.  Where the reference is not finite — the row
    without in-edges under max / min aggregates to NNlib's ∓Inf, and x̄ of that node follows — the same value is owed exactly"""
    assert np.shape(got) == np.shape(ref), what
    got, ref, same = R.split_nonfinite(got, ref)
    assert same, f"{what}: the reference's non-finite entries are not reproduced"
    assert np.all(np.isfinite(got)), f"{what}: non-finite"
    err, scale = np.linalg.norm(got - ref), np.linalg.norm(ref)
    worst = np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300) if ref.size else 0.0
    print(f"{what}: |got - ref| = {err:.3e}, |ref| = {scale:.3e}, ratio {err / max(scale, 1e-300):.2e}, element-wise {worst:.2e}")
    assert err <= tol * scale, f"{what}: {err:.3e} > {tol:g} * {scale:.3e}"
    assert worst <= tol, f"{what}: element-wise {worst:.2e} of the array scale"


def within_sum_bound(got, ref, mag, n, what):
    """|got − ref64| <= γ_n Σ|terms|, element-wise; the reference's non-finite entries (R.split_nonfinite) are owed exactly"""
    assert np.shape(got) == np.shape(ref), what
    got, ref, same = R.split_nonfinite(got, ref)
    assert same and np.all(np.isfinite(got)), f"{what}: the reference's non-finite entries are not reproduced"
    bound = R.gamma(n) * np.where(np.isfinite(mag), mag, 0.0)
    used = float((np.abs(got - ref) / np.maximum(bound, 1e-300)).max()) if got.size else 0.0
    print(f"{what}: uses {used:.3f} of the summation bound (n = {n})")
    assert np.all(np.abs(got - ref) <= bound), f"{what}: {used:.2f} of the summation bound"
    return used


def ptr(v):
    return None if v is None else ctypes.c_void_p(v.data_ptr())


def call_edge(lib, plan, P, Q, F, a0, z0, act, hid, stream=None):
    from gnnmp import _lib
    job = _lib.MegnetEdgeJob(P, Q, F, a0, z0, act)
    return lib.gnnmp_megnet_edge_f32(plan, ctypes.byref(job), hid, stream)


def call_grad(lib, plan, plan_t, da0, z, dz0, dP, dQ, act, hid, stream=None):
    from gnnmp import _lib
    job = _lib.MegnetEdgeGradJob(da0, z, dz0, dP, dQ, act)
    return lib.gnnmp_megnet_edge_grad_f32(plan, plan_t, ctypes.byref(job), hid, stream)


def call_agg(lib, plan, dy, m, y, acc, dm, aggr, D, stream=None):
    from gnnmp import _lib
    job = _lib.AggregateGradJob(dy, m, y, acc, dm)
    return lib.gnnmp_aggregate_grad_f32(plan, ctypes.byref(job), aggr, D, stream)


@pytest.fixture(scope="module")
def lib():
    import torch
    assert torch.cuda.is_available()
    from gnnmp import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def graph(lib):
    """the multigraph of tests/megnet_conv_ref.py as a GNNGraph with 0-based int64 indices"""
    import gnnmp
    s, t, tie = R.graph()
    R.assert_graph(s, t, tie)
    g = gnnmp.GNNGraph(dev(s), dev(t), num_nodes=R.N_NODES, index_base=0)
    g.plan(False), g.plan_transposed(False)
    return g, s, t, tie


def nan(*shape):
    import torch
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def run_edge(lib, g, case, name, with_F=True, want_z0=True):
    """(a0, z0 | None) as numpy arrays; outputs start as NaN"""
    import torch
    P, Q, F, _ = [dev(a) for a in case]
    E, hid = F.shape
    a0, z0 = nan(E, hid), nan(E, hid) if want_z0 else None
    rc = call_edge(lib, g.plan(False).handle, ptr(P), ptr(Q), ptr(F) if with_F else None, ptr(a0), ptr(z0), R.ACT_CODE[name], hid)
    assert rc == A.OK, lib.gnnmp_last_error()
    torch.cuda.synchronize()
    return a0.cpu().numpy(), None if z0 is None else z0.cpu().numpy()


def run_grad(lib, g, da0, z, name, want_dz0=True, want_nodes=True):
    """(dz0 | None, dP | None, dQ | None) as numpy arrays; outputs start as NaN"""
    import torch
    da0, z = dev(da0), None if z is None else dev(z)
    E, hid = da0.shape
    dz0 = nan(E, hid) if want_dz0 else None
    dP, dQ = (nan(R.N_NODES, hid), nan(R.N_NODES, hid)) if want_nodes else (None, None)
    rc = call_grad(lib, g.plan(False).handle, g.plan_transposed(False).handle if want_nodes else None, ptr(da0), ptr(z), ptr(dz0), ptr(dP),
                   ptr(dQ), R.ACT_CODE[name], hid)
    assert rc == A.OK, lib.gnnmp_last_error()
    torch.cuda.synchronize()
    return tuple(None if v is None else v.cpu().numpy() for v in (dz0, dP, dQ))


def run_agg(lib, g, case, aggr, with_acc=True, with_my=True):
    import torch
    dy, m, y, acc = [dev(a) for a in case]
    dm = nan(*m.shape)
    rc = call_agg(lib, g.plan(False).handle, ptr(dy), ptr(m) if with_my else None, ptr(y) if with_my else None, ptr(acc) if with_acc else None,
                  ptr(dm), R.AGGR_CODE[aggr], m.shape[1])
    assert rc == A.OK, lib.gnnmp_last_error()
    torch.cuda.synchronize()
    return dm.cpu().numpy()


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU 1: the exports against float64
# ------------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", R.ACTS)
@pytest.mark.parametrize("hid", R.WIDTHS)
def test_edge_exports_against_float64(lib, graph, hid, name):
    """hid = 1, 3, 7: 4-byte lanes; 2, 6: 8-byte lanes; 64, 100, 260: 16-byte lanes (100: 25 of 32 lanes active; 260: a second feature tile
    with one active lane).  a0, z0, dz0, dP, dQ within 1e-5 of float64 with and without F; a0 = gnnmp_bias_act_f32(z0) bit for bit;
    no optional output changes the bits of the others; rows without in-edges / out-edges get zeros; equal bits of two calls; for relu
    a0 serves as z; for identity z may be NULL"""
    import torch
    import gnnmp
    g, s, t, _ = graph
    case = R.edge_case(hid, name)
    for with_F in (True, False):
        a0_64, z0_64, dz0_64, dP_64, dQ_64 = R.edge_ref64(hid, name, with_F)
        a0, z0 = run_edge(lib, g, case, name, with_F)
        close(z0, z0_64, "z0")
        close(a0, a0_64, "a0")
        zt = dev(z0)
        want = zt if name == "identity" else gnnmp.layers_more._bias_act_code(zt, None, name)
        torch.cuda.synchronize()
        assert np.array_equal(bits(want.cpu().numpy()), bits(a0))
        a0_only, none = run_edge(lib, g, case, name, with_F, want_z0=False)
        assert none is None and np.array_equal(bits(a0_only), bits(a0))
        dz0, dP, dQ = run_grad(lib, g, case[3], z0, name)
        close(dz0, dz0_64, "dz0")
        close(dP, dP_64, "dP")
        close(dQ, dQ_64, "dQ")
        assert not dP[R.NO_IN].any() and not dQ[R.NO_OUT].any()
        dz0_b, none_p, none_q = run_grad(lib, g, case[3], z0, name, want_nodes=False)
        none_z, dP_b, dQ_b = run_grad(lib, g, case[3], z0, name, want_dz0=False)
        assert none_p is None and none_q is None and none_z is None
        assert np.array_equal(bits(dz0_b), bits(dz0)) and np.array_equal(bits(dP_b), bits(dP)) and np.array_equal(bits(dQ_b), bits(dQ))
        again = run_grad(lib, g, case[3], z0, name)
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(again, (dz0, dP, dQ)))
        if name == "relu":
            via_a0 = run_grad(lib, g, case[3], a0, name)
            assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(via_a0, (dz0, dP, dQ)))
        if name == "identity":
            no_z = run_grad(lib, g, case[3], None, name)
            assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(no_z, (dz0, dP, dQ)))
            assert np.array_equal(bits(dz0), bits(case[3]))


@gpu
@pytest.mark.parametrize("aggr", R.AGGRS)
@pytest.mark.parametrize("D", R.WIDTHS)
def test_aggregate_grad_against_float64(lib, graph, D, aggr):
    """dm within 1e-5 of float64 with and without acc; + and mean do not read m and y (NULL is taken); under max / min BOTH copies of the
    tied edge receive Δ in the channel where the tie wins; equal bits of two calls"""
    g, s, t, (k1, k2) = graph
    case = R.aggr_case(D, aggr)
    for with_acc in (True, False):
        dm = run_agg(lib, g, case, aggr, with_acc)
        close(dm, R.aggr_ref64(D, aggr, with_acc), "dm")
        assert np.array_equal(bits(run_agg(lib, g, case, aggr, with_acc)), bits(dm))
        if aggr in ("+", "mean"):
            assert np.array_equal(bits(run_agg(lib, g, case, aggr, with_acc, with_my=False)), bits(dm))
    if aggr in ("max", "min"):
        dy = case[0]
        assert dm[k1, 0] == dm[k2, 0] == dy[t[k1], 0] != 0      # (the last run was without acc)
    if aggr == "+":
        assert np.array_equal(bits(dm), bits(case[0][t]))


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU 2: the memory contract
# ------------------------------------------------------------------------------------------------------------------------------------
def contract_graph():
    s, t, _ = R.graph()
    return A.Graph("megnet", s + 1, t + 1, R.N_NODES)


def edge_arrays(case, with_F=True, with_z0=True):
    P, Q, F, _ = case
    arrs = [A.Arr("P", "in", P), A.Arr("Q", "in", Q)] + ([A.Arr("F", "in", F)] if with_F else [])
    return arrs + [A.Arr("a0", "out", shape=F.shape)] + ([A.Arr("z0", "out", shape=F.shape)] if with_z0 else [])


def edge_want(slab, hid, name, seed=0):
    a0, z0, *_ = R.edge_ref64(hid, name, "F" in slab.arrs, seed)
    return {k: v for k, v in {"a0": A.E(a0), "z0": A.E(z0)}.items() if k in slab.arrs}


def grad_inputs(hid, name, seed=0):
    """(da0, z): z = the float32 restatement of z0"""
    s, t, _ = R.graph()
    P, Q, F, da0 = R.edge_case(hid, name, seed)
    return da0, R.edge(s, t, P, Q, F, name)[1]


def grad_arrays(hid, name, want_dz0=True, want_nodes=True, seed=0):
    da0, z = grad_inputs(hid, name, seed)
    arrs = [A.Arr("da0", "in", da0), A.Arr("z", "in", z)] + ([A.Arr("dz0", "out", shape=z.shape)] if want_dz0 else [])
    return arrs + ([A.Arr("dP", "out", shape=(R.N_NODES, hid)), A.Arr("dQ", "out", shape=(R.N_NODES, hid))] if want_nodes else [])


def grad_want(slab, hid, name, seed=0):
    _, _, dz0, dP, dQ = R.edge_ref64(hid, name, True, seed)
    return {k: v for k, v in {"dz0": A.E(dz0), "dP": A.E(dP), "dQ": A.E(dQ)}.items() if k in slab.arrs}


def agg_arrays(case, with_acc=True):
    dy, m, y, acc = case
    arrs = [A.Arr("dy", "in", dy), A.Arr("m", "in", m), A.Arr("y", "in", y)] + ([A.Arr("acc", "in", acc)] if with_acc else [])
    return arrs + [A.Arr("dm", "out", shape=m.shape)]


def _p(slab):
    return lambda nm: slab.ptr(nm) if nm in slab.arrs else None


@gpu
@pytest.mark.parametrize("hid", [8, 6, 260])
def test_memory_contract_of_the_edge_exports(lib, hid):
    """every element of a0, z0, dz0, dP, dQ written — the rows without edges included — no store before or after an array or into an
    input, with each array in turn shifted to 16-, 8- and 4-byte alignment (hid = 8, 260: 16-byte lanes narrow to 8 and 4; hid = 6: 8-byte
    lanes narrow to 4), on a side stream, the hub rows included; once without F, without z0, with dz0 only, with dP and dQ only"""
    import torch
    side = torch.cuda.Stream()
    sp = ctypes.c_void_p(side.cuda_stream)
    plans = A.Plans(lib)
    g = contract_graph()
    try:
        plan, plan_t = plans.get(A.Pl(g)), plans.get(A.Pl(g, T=True))
        case = R.edge_case(hid, "relu")
        names = [a.name for a in edge_arrays(case)]
        runs = [({}, {})] + [({nm: A.SHIFTS[a]}, {}) for nm in names for a in ("a16", "a8", "a4")]
        runs += [({}, dict(with_F=False)), ({"P": 4}, dict(with_z0=False))]
        for k, (shifts, opts) in enumerate(runs):
            name = R.ACTS[k % 5]
            case = R.edge_case(hid, name)
            slab = A.Slab(edge_arrays(case, **opts), "cuda", shifts)
            p = _p(slab)
            torch.cuda.synchronize()
            rc = call_edge(lib, plan, p("P"), p("Q"), p("F"), p("a0"), p("z0"), R.ACT_CODE[name], hid, sp)
            torch.cuda.synchronize()
            assert rc == A.OK, (shifts, lib.gnnmp_last_error())
            problems = slab.check(edge_want(slab, hid, name))
            assert not problems, (name, shifts, opts, problems)
        names = [a.name for a in grad_arrays(hid, "relu")]
        runs = [({}, {})] + [({nm: A.SHIFTS[a]}, {}) for nm in names for a in ("a16", "a8", "a4")]
        runs += [({"z": 4}, dict(want_nodes=False)), ({"da0": 8}, dict(want_dz0=False))]
        for k, (shifts, opts) in enumerate(runs):
            name = R.ACTS[k % 5]
            slab = A.Slab(grad_arrays(hid, name, **opts), "cuda", shifts)
            p = _p(slab)
            torch.cuda.synchronize()
            rc = call_grad(lib, plan, plan_t, p("da0"), p("z"), p("dz0"), p("dP"), p("dQ"), R.ACT_CODE[name], hid, sp)
            torch.cuda.synchronize()
            assert rc == A.OK, (shifts, lib.gnnmp_last_error())
            problems = slab.check(grad_want(slab, hid, name))
            assert not problems, (name, shifts, opts, problems)
    finally:
        plans.close()


@gpu
@pytest.mark.parametrize("D", [8, 6, 260])
def test_memory_contract_of_the_aggregate_pullback(lib, D):
    """every element of dm written and nothing beyond, at every alignment of every array, for the four folds in turn, with and without acc"""
    import torch
    side = torch.cuda.Stream()
    sp = ctypes.c_void_p(side.cuda_stream)
    plans = A.Plans(lib)
    g = contract_graph()
    try:
        plan = plans.get(A.Pl(g))
        names = [a.name for a in agg_arrays(R.aggr_case(D, "+"))]
        runs = [({}, {})] + [({nm: A.SHIFTS[a]}, {}) for nm in names for a in ("a16", "a8", "a4")]
        runs += [({"m": 4}, dict(with_acc=False)), ({}, dict(with_acc=False)), ({"dm": 8}, dict(with_acc=False)), ({"dy": 4}, dict(with_acc=False))]
        for k, (shifts, opts) in enumerate(runs):
            aggr = R.AGGRS[k % 4]
            slab = A.Slab(agg_arrays(R.aggr_case(D, aggr), **opts), "cuda", shifts)
            p = _p(slab)
            torch.cuda.synchronize()
            rc = call_agg(lib, plan, p("dy"), p("m"), p("y"), p("acc"), p("dm"), R.AGGR_CODE[aggr], D, sp)
            torch.cuda.synchronize()
            assert rc == A.OK, (shifts, lib.gnnmp_last_error())
            problems = slab.check({"dm": A.E(R.aggr_ref64(D, aggr, "acc" in slab.arrs))})
            assert not problems, (aggr, shifts, opts, problems)
    finally:
        plans.close()


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU 3: capture, empty graphs
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
@pytest.mark.parametrize("which", ["edge", "grad", "aggregate"])
def test_the_exports_record_into_a_hip_graph_without_an_eager_call(lib, which):
    hid, name, aggr = 8, "swish", "max"
    g = contract_graph()
    plans = A.Plans(lib)
    seeds = (100, 101)
    try:
        plan, plan_t = plans.get(A.Pl(g)), plans.get(A.Pl(g, T=True))
        if which == "edge":
            cases = [R.edge_case(hid, name, sd) for sd in seeds]
            slab = A.Slab(edge_arrays(cases[0]))
            p = _p(slab)
            call = lambda sp: call_edge(lib, plan, p("P"), p("Q"), p("F"), p("a0"), p("z0"), R.ACT_CODE[name], hid, sp)      # noqa: E731
            reloads = [dict(zip(("P", "Q", "F"), case)) for case in cases]
            wants = [edge_want(slab, hid, name, sd) for sd in seeds]
        elif which == "grad":
            slab = A.Slab(grad_arrays(hid, name, seed=seeds[0]))
            p = _p(slab)
            call = lambda sp: call_grad(lib, plan, plan_t, p("da0"), p("z"), p("dz0"), p("dP"), p("dQ"), R.ACT_CODE[name], hid, sp)      # noqa: E731
            reloads = [dict(zip(("da0", "z"), grad_inputs(hid, name, sd))) for sd in seeds]
            wants = [grad_want(slab, hid, name, sd) for sd in seeds]
        else:
            cases = [R.aggr_case(hid, aggr, sd) for sd in seeds]
            slab = A.Slab(agg_arrays(cases[0]))
            p = _p(slab)
            call = lambda sp: call_agg(lib, plan, p("dy"), p("m"), p("y"), p("acc"), p("dm"), R.AGGR_CODE[aggr], hid, sp)      # noqa: E731
            reloads = [dict(zip(("dy", "m", "y", "acc"), case)) for case in cases]
            wants = [{"dm": A.E(R.aggr_ref64(hid, aggr, True, sd))} for sd in seeds]
        assert not np.array_equal(list(reloads[0].values())[0], list(reloads[1].values())[0])
        _capture_and_replay(lib, slab, call, reloads, wants)
    finally:
        plans.close()


@gpu
def test_empty_graphs(lib):
    """E = 0 with N > 0: dP and dQ are zeros and no E-row array is touched (their pointers are NULL here); the edge step and the aggregate
    pullback return OK without a launch"""
    import torch
    import gnnmp
    n, hid = 9, 6
    nothing = np.zeros(0, np.int64)
    g = gnnmp.GNNGraph(dev(nothing), dev(nothing), num_nodes=n, index_base=0)
    plan, plan_t = g.plan(False).handle, g.plan_transposed(False).handle
    PQ = dev(np.ones((n, hid), f32))
    assert call_edge(lib, plan, ptr(PQ), ptr(PQ), None, None, None, 1, hid) == A.OK
    dP, dQ = nan(n, hid), nan(n, hid)
    assert call_grad(lib, plan, plan_t, None, None, None, ptr(dP), ptr(dQ), 4, hid) == A.OK
    torch.cuda.synchronize()
    assert not dP.cpu().numpy().any() and not dQ.cpu().numpy().any()
    assert call_grad(lib, plan, None, None, None, ctypes.c_void_p(0x1000), None, None, 4, hid) == A.OK      # dz0 of no edge: not touched
    for aggr in range(4):
        assert call_agg(lib, plan, ptr(PQ), None, None, None, None, aggr, hid) == A.OK
    torch.cuda.synchronize()
    m = torch.zeros((0, hid), dtype=torch.float32, device="cuda", requires_grad=True)
    y = gnnmp.aggregate_neighbors_ad(g, "mean", m)
    y.sum().backward()
    assert y.shape == (n, hid) and m.grad.shape == (0, hid)


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU 4: the layer
# ------------------------------------------------------------------------------------------------------------------------------------
def make_layer(phi_e, phi_v, aggr):
    import gnnmp

    def chain(ch):
        out = []
        for W, b, a in ch:
            d = gnnmp.Dense((W.shape[1], W.shape[0]), a, bias=b is not None)
            d.weight = dev(W)
            if b is not None:
                d.bias = dev(b)
            out.append(d)
        return out
    return gnnmp.MEGNetConv(phi_e=chain(phi_e), phi_v=chain(phi_v), aggr=aggr)


def leaves(l):
    return [p for d in list(l.phi_e) + list(l.phi_v) for p in (d.weight, d.bias) if p is not None]


def layer_run(l, g, x, e, dxb, deb):
    """dict(xb, eb, dx, de, phi_e = [(dW, db)], phi_v) of megnet_conv_ad as numpy arrays; dxb / deb None: that output is left out of the loss"""
    import torch
    import gnnmp
    xt, et = dev(x).requires_grad_(True), dev(e).requires_grad_(True)
    for p in leaves(l):
        p.requires_grad_(True)
        p.grad = None
    xb, eb = gnnmp.megnet_conv_ad(l, g, xt, et)
    loss = sum((o * dev(d)).sum() for o, d in ((xb, dxb), (eb, deb)) if d is not None)
    loss.backward()
    torch.cuda.synchronize()
    np_ = lambda v: None if v is None else v.detach().cpu().numpy()      # noqa: E731
    grads = lambda ch: [(np_(d.weight.grad), None if d.bias is None else np_(d.bias.grad)) for d in ch]      # noqa: E731
    return dict(xb=np_(xb), eb=np_(eb), dx=np_(xt.grad), de=np_(et.grad), phi_e=grads(l.phi_e), phi_v=grads(l.phi_v))


@gpu
@pytest.mark.parametrize("shape,aggr", LAYER_CASES)
def test_layer_forward(graph, shape, aggr):
    """x̄ and ē of megnet_conv_ad within 1e-5 of the float64 reference, of oracle.more_layers.megnet_conv and of gnnmp.megnet_conv, with the
    default chains; under no_grad the same bits"""
    import torch
    import gnnmp
    g, s, t, _ = graph
    x, e, phi_e, phi_v, _, _ = R.layer_case(shape, aggr)
    l = make_layer(phi_e, phi_v, aggr)
    ref = R.layer_ref64(shape, aggr, "both")
    with torch.no_grad():
        xb, eb = gnnmp.megnet_conv_ad(l, g, dev(x), dev(e))
        xb_p, eb_p = gnnmp.megnet_conv(l, g, dev(x), dev(e))
    xb_o, eb_o = _oracle(shape, aggr)
    xb, eb = xb.cpu().numpy(), eb.cpu().numpy()
    for what, a, b in (("x̄", xb, ref["xb"]), ("ē", eb, ref["eb"]), ("x̄ / oracle", xb, xb_o), ("ē / oracle", eb, eb_o),
                       ("x̄ / megnet_conv", xb, xb_p.cpu().numpy()), ("ē / megnet_conv", eb, eb_p.cpu().numpy())):
        close(a, b, what)
    xt = dev(x).requires_grad_(True)
    xb2, eb2 = gnnmp.megnet_conv_ad(l, g, xt, dev(e))
    assert xb2.requires_grad and eb2.requires_grad
    assert np.array_equal(bits(xb2.detach().cpu().numpy()), bits(xb)) and np.array_equal(bits(eb2.detach().cpu().numpy()), bits(eb))


@gpu
@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("shape,aggr", LAYER_CASES)
def test_layer_gradients(graph, shape, aggr, mode):
    """loss on x̄ only, ē only, or both: dx and de within 1e-5; every weight and bias gradient inside γ_n Σ|terms| of the float64 reference
    (n = E, the longest fold on the path to either chain's terms: R.grad).  WORST OBSERVED FRACTION OF THE BOUND: LABNOTES.md"""
    g, s, t, _ = graph
    x, e, phi_e, phi_v, dxb, deb = R.layer_case(shape, aggr)
    ref = R.layer_ref64(shape, aggr, mode)
    l = make_layer(phi_e, phi_v, aggr)
    got = layer_run(l, g, x, e, dxb if mode in ("x", "both") else None, deb if mode in ("e", "both") else None)
    close(got["dx"], ref["dx"], "dx")
    close(got["de"], ref["de"], "de")
    used = 0.0
    for cname, mname, n in (("phi_e", "mag_e", ref["n_e"]), ("phi_v", "mag_v", ref["n_v"])):
        for q, (dW, db) in enumerate(got[cname]):
            if ref[cname][q] is None:                      # mode e: ϕv does not reach the loss
                assert mode == "e" and cname == "phi_v" and dW is None and db is None
                continue
            used = max(used, within_sum_bound(dW, ref[cname][q][0], ref[mname][q][0], n, f"{cname}[{q}].weight"))
            used = max(used, within_sum_bound(db, ref[cname][q][1], ref[mname][q][1], n, f"{cname}[{q}].bias"))
    print(f"worst fraction of the summation bound: {used:.3f}")


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU 5: behaviour
# ------------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", ["relu", "tanh"])
def test_needs_input_grad_prunes(graph, name):
    """only x needs a gradient: no dz0 is allocated; relu keeps no z0 (a0 serves as z), tanh does; dx still within 1e-5"""
    import torch
    import gnnmp
    from gnnmp import backward_megnet as B
    g, s, t, _ = graph
    shape, aggr = (12, 16), "mean"
    x, e, phi_e, phi_v, dxb, deb = R.layer_case(shape, aggr, act0=name)
    l = make_layer(phi_e, phi_v, aggr)
    seen_grad, seen_edge = [], []
    grad_fn, edge_fn = B.megnet_edge_grad, B.megnet_edge
    B.megnet_edge_grad = lambda *a: seen_grad.append(a[5:]) or grad_fn(*a)
    B.megnet_edge = lambda *a: seen_edge.append(a[5]) or edge_fn(*a)
    try:
        xt = dev(x).requires_grad_(True)
        xb, eb = gnnmp.megnet_conv_ad(l, g, xt, dev(e))
        ((xb * dev(dxb)).sum() + (eb * dev(deb)).sum()).backward()
        torch.cuda.synchronize()
    finally:
        B.megnet_edge_grad, B.megnet_edge = grad_fn, edge_fn
    assert seen_grad == [(False, True)] and seen_edge == [name != "relu"]      # (want_dz0, want_nodes); want_z0
    assert all(p.grad is None for p in leaves(l))
    s_, t_, _ = R.graph()
    c64 = R._cast((x, e, phi_e, phi_v, dxb, deb), f64)
    close(xt.grad.cpu().numpy(), R.grad(s_, t_, R.N_NODES, *c64[:4], aggr, c64[4], c64[5])["dx"], "dx")


@gpu
def test_megnet_conv_ad_refuses_by_name(graph):
    import torch
    import gnnmp
    g, _, _, _ = graph
    x, e, phi_e, phi_v, _, _ = R.layer_case((7, 5), "+")
    l = make_layer(phi_e, phi_v, "+")
    xt, et = dev(x), dev(e)
    with pytest.raises(NotImplementedError, match="bipartite"):
        gnnmp.megnet_conv_ad(l, g, (xt, xt), et)
    with pytest.raises(ValueError, match="the first ϕe weight has 21 columns, 2 in \\+ ein = 20"):
        gnnmp.megnet_conv_ad(l, g, xt, et[:, :6].contiguous())
    with pytest.raises(ValueError, match="the first ϕe weight has 21 columns, 2 in \\+ ein = 19"):
        gnnmp.megnet_conv_ad(l, g, xt[:, :6].contiguous(), et)
    narrow = make_layer(phi_e, [(phi_v[0][0][:, :-1], phi_v[0][1], "relu"), phi_v[1]], "+")
    with pytest.raises(ValueError, match="the first ϕv weight has 11 columns"):
        gnnmp.megnet_conv_ad(narrow, g, xt, et)

    class NotDense:
        pass
    for chains in (dict(phi_e=[l.phi_e[0], NotDense()], phi_v=l.phi_v), dict(phi_e=l.phi_e, phi_v=[NotDense(), l.phi_v[1]])):
        with pytest.raises(TypeError, match="NotDense"):
            gnnmp.megnet_conv_ad(gnnmp.MEGNetConv(aggr="+", **chains), g, xt, et)
    for name in R.ACTS:      # ϕe's first layer takes all five
        ok = make_layer([(phi_e[0][0], phi_e[0][1], name), phi_e[1]], phi_v, "+")
        gnnmp.megnet_conv_ad(ok, g, xt, et)
    for bad in (make_layer([phi_e[0], (phi_e[1][0], phi_e[1][1], "tanh")], phi_v, "+"),
                make_layer(phi_e, [(phi_v[0][0], phi_v[0][1], "swish"), phi_v[1]], "+")):
        with pytest.raises(ValueError, match="identity and relu"):
            gnnmp.megnet_conv_ad(bad, g, xt, et)
    with pytest.raises(ValueError, match="not in the gnnmp_act set"):
        gnnmp.megnet_conv_ad(make_layer([(phi_e[0][0], phi_e[0][1], torch.tanh), phi_e[1]], phi_v, "+"), g, xt, et)
    torch.cuda.synchronize()


@gpu
@pytest.mark.parametrize("aggr", R.AGGRS)
def test_aggregate_neighbors_ad(graph, aggr):
    """forward: gnnmp.aggregate_neighbors bit for bit; backward: the reference's pullback"""
    import torch
    import gnnmp
    g, s, t, _ = graph
    D = 7
    dy, m, y, _ = R.aggr_case(D, aggr)
    mt = dev(m).requires_grad_(True)
    out = gnnmp.aggregate_neighbors_ad(g, aggr, mt)
    plain = gnnmp.aggregate_neighbors(g, aggr, dev(m))
    out.backward(dev(dy))
    torch.cuda.synchronize()
    assert np.array_equal(bits(out.detach().cpu().numpy()), bits(plain.cpu().numpy()))
    close(out.detach().cpu().numpy(), R.aggregate(t, R.N_NODES, m.astype(f64), aggr), "y")
    close(mt.grad.cpu().numpy(), R.aggr_ref64(D, aggr, False), "dm")


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU 6: a MEGNet step
# ------------------------------------------------------------------------------------------------------------------------------------
@gpu
def test_a_two_layer_megnet_step():
    """radius_graph on one cloud of 256 points -> e = 8 Gaussian basis functions of the edge length -> MEGNetConv(8 => 16),
    MEGNetConv(16 => 16) (the second takes the first's x̄ AND ē, projected back to 16 edge features by construction) -> loss = mean x̄² +
    mean ē²: every parameter gets a finite, non-zero gradient, and one plain SGD step lowers the loss"""
    import torch
    import gnnmp
    c = R.MEGNET
    rng = np.random.default_rng(c["seed"])
    pos = dev(rng.uniform(0, 1, (c["pts"], 3)).astype(f32))
    g = gnnmp.radius_graph(pos, c["radius"])
    assert g.num_edges > c["pts"]
    d = (pos[g.s - 1] - pos[g.t - 1]).norm(dim=1, keepdim=True)
    mu = torch.linspace(0, c["radius"], c["centers"], device="cuda")[None, :]
    e = torch.exp(-((d - mu) / (c["radius"] / c["centers"])) ** 2).contiguous().requires_grad_(True)
    x = dev(rng.standard_normal((c["pts"], c["nin"])).astype(f32)).requires_grad_(True)
    layers = [gnnmp.MEGNetConv((c["nin"], c["hid"]), seed=11), gnnmp.MEGNetConv((c["hid"], c["hid"]), seed=21)]
    params = [p for l in layers for p in leaves(l)]
    for l in layers:
        for dn in list(l.phi_e) + list(l.phi_v):
            dn.bias.data.fill_(0.05)
    for p in params:
        p.requires_grad_(True)

    def loss():
        h, eb = gnnmp.megnet_conv_ad(layers[0], g, x, e)
        h, eb = gnnmp.megnet_conv_ad(layers[1], g, h, eb)
        return (h ** 2).mean() + (eb ** 2).mean()
    before = loss()
    before.backward()
    before = before.detach()
    torch.cuda.synchronize()
    for v in params + [x, e]:
        assert v.grad is not None and bool(torch.isfinite(v.grad).all()) and bool((v.grad != 0).any())
    gsq = sum(float((p.grad.double() ** 2).sum()) for p in params)
    lr = 0.05 * float(before) / gsq          # a step that would cut a linear loss by 5 %
    with torch.no_grad():
        for p in params:
            p -= lr * p.grad
        after = loss()
    print(f"loss {float(before):.6f} -> {float(after):.6f} (lr {lr:.3e})")
    assert float(after) < float(before)
