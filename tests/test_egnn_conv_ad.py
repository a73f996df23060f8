"""egnn_conv_ad: EGNNConv trained on the fused coordinate kernels (csrc/egnn.hip; include/gnnmp.h states the arithmetic).

Without a GPU: the four exports exist in header, SYMBOLS and library and take const plans and const host records whose ctypes layouts are
the header's; every refusal of the header comes before any HIP call; the float64 gradient reference (tests/egnn_conv_ref.py) agrees with
central finite differences for every operand and all five activations; the operands of every GPU case keep the float32 restatement
within 2e-6 of float64 and, for relu, away from the kink.

On the GPU: K1 (q, z0, a0) at every lane width, tail and tile count, K2 (x') and K3 (dmx, dx; three ways, equal bits) at every coordinate
capacity, act'(z) for all five codes, within 1e-5 of float64, on a multigraph of 700 nodes with a self loop, repeated edges, a coincident
pair, a row without in-edges, a row without out-edges and a hub destination and source of 600 edges; the layer's h', x' and every
gradient within 1e-5 of the reference, h' and x' also of oracle.more_layers.egnn_conv and gnnmp.egnn_conv; every output element written
and nothing else (the slab of tests/abi_cases.py) at any pointer alignment; each export recorded into a HIP graph without an eager call
first; two calls give equal bits; empty graphs; the refusals of egnn_conv_ad; a small EGNN step on a device-built radius graph."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_cases as A  # noqa: E402
import egnn_conv_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EDGE, COORD, COORD_GRAD, ACT_Z = "gnnmp_egnn_edge_f32", "gnnmp_egnn_coord_f32", "gnnmp_egnn_coord_grad_f32", "gnnmp_act_grad_z_f32"
EXPORTS = (EDGE, COORD, COORD_GRAD, ACT_Z)
RECORDS = {      # export -> (struct of the header, ctypes class, fields, offsets, size)
    EDGE: ("gnnmp_egnn_edge_t", "EgnnEdgeJob", ("s", "t", "idx_bytes", "index_base", "x", "P", "Q", "F", "c", "q", "a0", "z0", "act"),
           [0, 8, 16, 20, 24, 32, 40, 48, 56, 64, 72, 80, 88], 96),
    COORD: ("gnnmp_egnn_coord_t", "EgnnCoordJob", ("x", "mx", "xo"), [0, 8, 16], 24),
    COORD_GRAD: ("gnnmp_egnn_coord_grad_t", "EgnnCoordGradJob", ("x", "dxo", "mx", "dq", "dmx", "dx"), [0, 8, 16, 24, 32, 40], 48),
    ACT_Z: ("gnnmp_act_grad_z_t", "ActGradZJob", ("dy", "z", "dz", "act"), [0, 8, 16, 24], 32),
}
PARAMS = {EDGE: ["job", "E", "hid", "Dx", "stream"], COORD: ["plan", "job", "Dx", "stream"],
          COORD_GRAD: ["plan", "plan_t", "job", "Dx", "stream"], ACT_Z: ["job", "n", "stream"]}
gpu = pytest.mark.gpu
f32, f64 = np.float32, np.float64


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
    for name in EXPORTS:
        assert f"int {name}(" in header and header.index(f"int {name}(") < internal, name
        assert name in _lib.SYMBOLS and name in exported, name
        assert "} %s;" % RECORDS[name][0] in header
    assert "GNNlib/src/layers/conv.jl:459-495" in header[:internal]
    assert "tests/test_egnn_conv_ad.py" in header[:header.index("#ifndef GNNMP_H")]           # the Conventions paragraph: what is tested
    assert "q_k == 0" in header[:internal] and "Inf * 0" in header[:internal]                 # the convention is stated
    assert callable(gnnmp.egnn_conv_ad)


def test_the_exports_take_const_plans_and_const_host_records():
    """device pointers travel in const host records: the table of tests/abi_cases.py owes no case, this file carries the memory-contract
    and capture checks itself.  The ctypes records have the layouts of the header's structs."""
    from gnnmp import _lib
    decls, _ = A.parse_header()
    owed = A.must_be_covered(decls, _lib.SYMBOLS)
    header = open(os.path.join(ROOT, "include", "gnnmp.h")).read()
    for name in EXPORTS:
        assert name not in owed
        assert [p[0] for p in decls[name]] == PARAMS[name]
        for pname, is_ptr, is_const, _ in decls[name]:
            assert is_const or not is_ptr, (name, pname)
        struct, cls, want_fields, want_offsets, size = RECORDS[name]
        body = re.search(r"typedef struct \{([^}]*)\} %s;" % struct, header).group(1)
        body = re.sub(r"/\*.*?\*/", " ", body, flags=re.S)
        fields, off, offsets = [], 0, []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            is_ptr = "*" in decl
            names = [n.strip().lstrip("*") for n in re.sub(r"^(const\s+)?(float|int|void)\s+", "", decl).split(",")]
            for nme in names:
                sz = 8 if is_ptr else 4
                off = (off + sz - 1) // sz * sz
                fields.append(nme)
                offsets.append(off)
                off += sz
        rec = getattr(_lib, cls)
        assert tuple(fields) == want_fields, name
        assert [getattr(rec, f).offset for f in fields] == offsets == want_offsets, name
        assert ctypes.sizeof(rec) == size == (off + 7) // 8 * 8, name


P = lambda v: ctypes.c_void_p(0x1000 * v) if v else None      # never dereferenced: the call must refuse first  # noqa: E731


class _FakePlan(ctypes.Structure):
    """the head of csrc/common.h's gnnmp_graph {int64 n_src, n_dst, n_edges, n_total; ...}: all the refusals read of a plan"""
    _fields_ = [("n_src", ctypes.c_int64), ("n_dst", ctypes.c_int64), ("n_edges", ctypes.c_int64), ("n_total", ctypes.c_int64),
                ("tail", ctypes.c_char * 1024)]


def _edge(lib, job=True, s=1, t=2, idx_bytes=8, x=3, Pm=4, Q=5, F=6, c=7, q=8, a0=9, z0=10, act=4, E=7, hid=4, Dx=3):
    from gnnmp import _lib
    j = _lib.EgnnEdgeJob(P(s), P(t), idx_bytes, 0, P(x), P(Pm), P(Q), P(F), P(c), P(q), P(a0), P(z0), act)
    return lib.gnnmp_egnn_edge_f32(ctypes.byref(j) if job else None, E, hid, Dx, None)


def _coord(lib, plan, job=True, x=1, mx=2, xo=3, Dx=3):
    from gnnmp import _lib
    j = _lib.EgnnCoordJob(P(x), P(mx), P(xo))
    return lib.gnnmp_egnn_coord_f32(plan, ctypes.byref(j) if job else None, Dx, None)


def _coord_grad(lib, plan, plan_t, job=True, x=1, dxo=2, mx=3, dq=4, dmx=5, dx=6, Dx=3):
    from gnnmp import _lib
    j = _lib.EgnnCoordGradJob(P(x), P(dxo), P(mx), P(dq), P(dmx), P(dx))
    return lib.gnnmp_egnn_coord_grad_f32(plan, plan_t, ctypes.byref(j) if job else None, Dx, None)


def _act_z(lib, job=True, dy=1, z=2, dz=3, act=4, n=5):
    from gnnmp import _lib
    j = _lib.ActGradZJob(P(dy), P(z), P(dz), act)
    return lib.gnnmp_act_grad_z_f32(ctypes.byref(j) if job else None, n, None)


def test_argument_validation_needs_no_gpu():
    """every refusal of the header comes before the first HIP call: on a machine without a device, on pointers that are not memory"""
    from gnnmp import _lib
    lib = _lib.load()
    EINVAL, OK, err = _lib.EINVAL, _lib.OK, lib.gnnmp_last_error
    mk = lambda **k: _FakePlan(**k)      # noqa: E731
    sq, sq_t = mk(n_src=5, n_dst=5, n_edges=7, n_total=7), mk(n_src=5, n_dst=5, n_edges=7, n_total=7)
    pl, pt = ctypes.addressof(sq), ctypes.addressof(sq_t)
    rect, tall = mk(n_src=9, n_dst=5, n_edges=7, n_total=7), mk(n_src=6, n_dst=6, n_edges=7, n_total=7)
    more, loops = mk(n_src=5, n_dst=5, n_edges=8, n_total=8), mk(n_src=5, n_dst=5, n_edges=7, n_total=12)
    none = mk(n_src=0, n_dst=0, n_edges=0, n_total=0)
    adr = ctypes.addressof
    # K1
    assert _edge(lib, job=False) == EINVAL and b"null job" in err()
    for name in ("s", "t", "x", "Pm", "Q", "c", "q", "a0"):
        assert _edge(lib, **{name: None}) == EINVAL and f"null {name.rstrip('m')}".encode() in err(), name
    assert _edge(lib, idx_bytes=2) == EINVAL and b"bad idx_bytes" in err()
    assert _edge(lib, E=-1) == EINVAL and b"negative E" in err()
    for hid in (0, -3, (1 << 19) + 1, 2 ** 40):
        assert _edge(lib, hid=hid) == EINVAL and b"bad hid" in err(), hid
    for Dx in (0, -1, 17, 2 ** 33):
        assert _edge(lib, Dx=Dx) == EINVAL and b"bad Dx" in err(), Dx
    for act in (-1, 5, 17):
        assert _edge(lib, act=act) == EINVAL and b"bad act" in err(), act
    assert _edge(lib, E=0) == OK and _edge(lib, E=0, F=None, z0=None, hid=1 << 19, Dx=16, act=0) == OK      # E = 0 launches nothing
    # K2
    assert _coord(lib, None) == EINVAL and b"null plan" in err()
    assert _coord(lib, pl, job=False) == EINVAL and b"null job" in err()
    for name in ("x", "mx", "xo"):
        assert _coord(lib, pl, **{name: None}) == EINVAL and f"null {name}".encode() in err(), name
    for Dx in (0, -1, 17, 2 ** 33):
        assert _coord(lib, pl, Dx=Dx) == EINVAL and b"bad Dx" in err(), Dx
    assert _coord(lib, adr(rect)) == EINVAL and b"not square" in err()
    assert _coord(lib, adr(loops)) == EINVAL and b"self loops" in err()
    assert _coord(lib, adr(none)) == OK                                                # N = 0 launches nothing
    # K3
    assert _coord_grad(lib, None, pt) == EINVAL and b"null plan" in err()
    assert _coord_grad(lib, pl, pt, job=False) == EINVAL and b"null job" in err()
    for name in ("x", "dxo"):
        assert _coord_grad(lib, pl, pt, **{name: None}) == EINVAL and f"null {name}".encode() in err(), name
    assert _coord_grad(lib, pl, pt, dmx=None, dx=None) == EINVAL and b"both null" in err()
    assert _coord_grad(lib, pl, None) == EINVAL and b"dx without plan_t" in err()
    assert _coord_grad(lib, pl, pt, mx=None) == EINVAL and b"dx without mx" in err()
    assert _coord_grad(lib, pl, pt, dq=None) == EINVAL and b"dx without dq" in err()
    for Dx in (0, -1, 17, 2 ** 33):
        assert _coord_grad(lib, pl, pt, Dx=Dx) == EINVAL and b"bad Dx" in err(), Dx
    assert _coord_grad(lib, adr(rect), pt) == EINVAL and b"not square" in err()
    assert _coord_grad(lib, pl, adr(tall)) == EINVAL and b"the transposed plan has 6 rows, the plan 5" in err()
    assert _coord_grad(lib, pl, adr(more)) == EINVAL and b"the transposed plan has 8 edges, the plan 7" in err()
    assert _coord_grad(lib, adr(loops), adr(loops)) == EINVAL and b"self loops" in err()
    assert _coord_grad(lib, adr(none), adr(none)) == OK
    assert _coord_grad(lib, adr(none), None, mx=None, dq=None, dx=None, Dx=16) == OK    # dmx only needs neither plan_t nor mx, dq
    # act'(z)
    assert _act_z(lib, job=False) == EINVAL and b"null job" in err()
    assert _act_z(lib, n=-1) == EINVAL and b"negative n" in err()
    for act in (-1, 5, 17):
        assert _act_z(lib, act=act) == EINVAL and b"bad act" in err(), act
    for name in ("dy", "dz", "z"):
        assert _act_z(lib, **{name: None}) == EINVAL and f"null {name}".encode() in err(), name
    assert _act_z(lib, n=0) == OK and _act_z(lib, n=0, z=None, act=0) == OK


# ------------------------------------------------------------------------------------------------------------------------------------
# CPU: the references
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.ACTS)
def test_reference_gradient_agrees_with_finite_differences(name):
    """central differences of the float64 layer, h = 1e-6, bar 1e-6 max(|g|, 1) (tests/test_cg_conv_ad.py): n = 12, E = 40, nin = 4,
    ein = 2, hid = 5, Dx = 3, residual on; `name` is the activation of both ϕe layers; relu's inputs are kept off the kink; no edge has
    q = 0 (the convention there is not a derivative)"""
    hh = 1e-6
    s, t, n, h, x, e, pe, px, ph, dhn, dxo = R.fd_case(name)
    fw = R.forward(s, t, n, h, x, e, pe, px, ph, True, f64)
    assert fw["q"].min() > 0.01
    if name == "relu":
        assert np.abs(fw["relu_pre"]).min() > 100 * hh
    bw = R.backward(fw, dhn, dxo)

    def loss():
        f = R.forward(s, t, n, h, x, e, pe, px, ph, True, f64)
        return float((f["hn"] * dhn).sum() + (f["xo"] * dxo).sum())

    operands = [(h, bw["dh"], "dh"), (x, bw["dx"], "dx"), (e, bw["de"], "de")]
    for chain_name, chain in (("phi_e", pe), ("phi_x", px), ("phi_h", ph)):
        for k, (W, b, _) in enumerate(chain):
            operands.append((W, bw[chain_name][k][0], f"dW {chain_name}[{k}]"))
            if b is not None:
                operands.append((b, bw[chain_name][k][1], f"db {chain_name}[{k}]"))
    assert len(operands) == 3 + 6 + 5
    for arr, g, what in operands:
        fd = np.zeros_like(arr)
        for i in np.ndindex(arr.shape):
            keep = arr[i]
            arr[i] = keep + hh
            hi = loss()
            arr[i] = keep - hh
            lo = loss()
            arr[i] = keep
            fd[i] = (hi - lo) / (2 * hh)
        assert np.abs(fd - g).max() <= 1e-6 * max(np.abs(g).max(), 1.0), (what, np.abs(fd - g).max())


def test_the_graph_has_what_the_tests_need():
    s, t = R.graph()
    R.assert_graph(s, t)
    for Dx in R.DXS:
        x = R.coords(Dx).astype(f64)
        q = ((x[t] - x[s]) ** 2).sum(axis=1)
        zero = R.q_zero(s, t)
        assert zero.sum() == 3 and not q[zero].any() and np.sqrt(q[~zero].min()) >= 0.3 - 1e-6, Dx


EDGE_CASES = [(hid, R.ACTS[(2 * k + int(wf)) % 5], wf) for k, hid in enumerate(R.HIDS) for wf in (False, True)]


def _assert_conditioned(what, cond):
    worst, ratio = cond
    assert worst <= R.COND, f"{what}: the float32 restatement is {worst:.2e} from float64 (bound {R.COND:g})"
    assert ratio >= R.MARGIN, f"{what}: a relu pre-activation is only {ratio:.1f} x the float32-float64 deviation of its row from 0"


def test_every_activation_is_an_edge_case():
    assert {name for _, name, _ in EDGE_CASES} == set(R.ACTS) and {h for h, _, _ in EDGE_CASES} == set(R.HIDS)


@pytest.mark.parametrize("hid,name,with_f", EDGE_CASES)
def test_the_edge_cases_are_well_conditioned(hid, name, with_f):
    """THE CONDITION ON THE INPUTS, not a measurement: q, z0, a0 evaluated in float32 by the header's formulas are within 2e-6, norm-wise,
    of float64 — a fifth of the 1e-5 bar.  (relu is continuous: K1 computes no derivative, there is no kink to stay away from.)"""
    s, t = R.graph()
    case = R.edge_case(hid, name, with_f)
    got, ref = R.edge_ref(s, t, *case, name, f32), R.edge_ref(s, t, *case, name)
    _assert_conditioned("edge case", R.condition(dict(enumerate(got)), dict(enumerate(ref))))


@pytest.mark.parametrize("Dx", R.DXS)
def test_the_coordinate_cases_are_well_conditioned(Dx):
    s, t = R.graph()
    x, dxo, mx, dq = R.coord_case(Dx)
    n = R.N_NODES
    got = (R.coord_ref(s, t, n, x, mx, f32),) + R.coord_grad_ref(s, t, n, x, dxo, mx, dq, f32)
    ref = (R.coord_ref(s, t, n, x, mx),) + R.coord_grad_ref(s, t, n, x, dxo, mx, dq)
    _assert_conditioned("coordinate case", R.condition(dict(enumerate(got)), dict(enumerate(ref))))


@pytest.mark.parametrize("name", R.ACTS)
@pytest.mark.parametrize("n", R.ACT_NS)
def test_the_activation_cases_are_well_conditioned(n, name):
    dy, z = R.act_case(n, name)
    _assert_conditioned("act'(z) case", R.condition({0: R.act_grad_z_ref(dy, z, name, f32)}, {0: R.act_grad_z_ref(dy, z, name)}))


@pytest.mark.parametrize("shape,residual", R.LAYER_CASES)
def test_the_layer_cases_are_well_conditioned(shape, residual):
    s, t = R.graph()
    _assert_conditioned("layer case", R.layer_condition(s, t, R.N_NODES, R.layer_case(shape), residual))


def test_the_training_step_is_well_conditioned():
    """on the CPU's own radius graph of the step's clouds (the device builds the same one: no pair lies within 1e-4 of the radius)"""
    pos, gi, h, layers, Rm, Rx = R.step_case()
    d = np.linalg.norm(pos[:, None].astype(f64) - pos[None].astype(f64), axis=2)
    adj = (d <= R.STEP["radius"]) & (gi[:, None] == gi[None]) & ~np.eye(len(pos), dtype=bool)
    assert np.abs(d[gi[:, None] == gi[None]] - R.STEP["radius"]).min() > 1e-4
    t, s = np.nonzero(adj)
    n = len(pos)
    fw1 = R.forward(s, t, n, h, pos, None, *layers[0], True, f32)
    fw2 = R.forward(s, t, n, fw1["hn"], fw1["xo"], None, *layers[1], True, f32)
    cnt = np.bincount(gi, minlength=Rm.shape[0])
    b2 = R.backward(fw2, (Rm / cnt[:, None].astype(f32))[gi], Rx)
    b1 = R.backward(fw1, b2["dh"], b2["dx"])
    h2, x2, grads, dh, dpos = R.step_grad64(s, t, gi, h, pos, layers, Rm, Rx)
    got = dict(h2=fw2["hn"], x2=fw2["xo"], dh=b1["dh"], dpos=b1["dx"], **{f"1 {k}": v for k, v in R.flat(fw1, b1).items() if k[0] == "d"},
               **{f"2 {k}": v for k, v in R.flat(fw2, b2).items() if k[0] == "d"})
    ref = dict(h2=h2, x2=x2, dh=dh, dpos=dpos)
    fws = (R.forward(s, t, n, h, pos, None, *layers[0], True, f64), None)
    ref.update({f"1 {k}": v for k, v in R.flat(fws[0], grads[0]).items() if k[0] == "d"})
    fw2_64 = R.forward(s, t, n, fws[0]["hn"], fws[0]["xo"], None, *layers[1], True, f64)
    ref.update({f"2 {k}": v for k, v in R.flat(fw2_64, grads[1]).items() if k[0] == "d"})
    _assert_conditioned("training step", R.condition(got, ref))


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


@pytest.fixture(scope="module")
def lib():
    import torch
    assert torch.cuda.is_available()
    from gnnmp import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def graph(lib):
    """the multigraph of tests/egnn_conv_ref.py as a GNNGraph with 0-based int64 indices; its properties, and that both plans DO split the
    hub rows (the scatters meet chunked rows, K2 / K3 walk them whole)"""
    import gnnmp
    s, t = R.graph()
    R.assert_graph(s, t)
    g = gnnmp.GNNGraph(dev(s), dev(t), num_nodes=R.N_NODES, index_base=0)
    plan, plan_t = g.plan(False), g.plan_transposed(False)
    assert R.HUB > plan.long_thresh == plan_t.long_thresh and plan.n_long >= 1 and plan_t.n_long >= 1
    return g, s, t


def nan_like(shape):
    import torch
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def run_edge(lib, g, case, name, want_z0=True):
    """(q, z0 | None, a0) of K1 as numpy arrays; outputs start as NaN"""
    import torch
    from gnnmp import _lib
    x, Pm, Q, F, c = [None if a is None else dev(a) for a in case]
    E, hid = g.num_edges, Pm.shape[1]
    q, a0 = nan_like((E,)), nan_like((E, hid))
    z0 = nan_like((E, hid)) if want_z0 else None
    job = _lib.EgnnEdgeJob(ptr(g.s), ptr(g.t), 8, 0, ptr(x), ptr(Pm), ptr(Q), ptr(F), ptr(c), ptr(q), ptr(a0), ptr(z0), R.ACT_CODE[name])
    assert lib.gnnmp_egnn_edge_f32(ctypes.byref(job), E, hid, x.shape[1], None) == A.OK, lib.gnnmp_last_error()
    torch.cuda.synchronize()
    return tuple(None if v is None else v.cpu().numpy() for v in (q, z0, a0))


def run_coord(lib, g, x, mx):
    import torch
    from gnnmp import _lib
    xd, mxd = dev(x), dev(mx)
    xo = nan_like(x.shape)
    job = _lib.EgnnCoordJob(ptr(xd), ptr(mxd), ptr(xo))
    assert lib.gnnmp_egnn_coord_f32(g.plan(False).handle, ctypes.byref(job), x.shape[1], None) == A.OK, lib.gnnmp_last_error()
    torch.cuda.synchronize()
    return xo.cpu().numpy()


def run_coord_grad(lib, g, x, dxo, mx, dq, want_dmx, want_dx):
    """(dmx | None, dx | None) of K3; a dmx-only call passes neither plan_t nor mx, dq"""
    import torch
    from gnnmp import _lib
    xd, dd = dev(x), dev(dxo)
    mxd, dqd = (dev(mx), dev(dq)) if want_dx else (None, None)
    dmx = nan_like((g.num_edges,)) if want_dmx else None
    dx = nan_like(x.shape) if want_dx else None
    job = _lib.EgnnCoordGradJob(ptr(xd), ptr(dd), ptr(mxd), ptr(dqd), ptr(dmx), ptr(dx))
    plan_t = g.plan_transposed(False).handle if want_dx else None
    assert lib.gnnmp_egnn_coord_grad_f32(g.plan(False).handle, plan_t, ctypes.byref(job), x.shape[1], None) == A.OK, lib.gnnmp_last_error()
    torch.cuda.synchronize()
    return tuple(None if v is None else v.cpu().numpy() for v in (dmx, dx))


def run_act_z(lib, dy, z, name):
    import torch
    from gnnmp import _lib
    dyd, zd = dev(dy), dev(z)
    dz = nan_like(dy.shape)
    job = _lib.ActGradZJob(ptr(dyd), ptr(zd), ptr(dz), R.ACT_CODE[name])
    assert lib.gnnmp_act_grad_z_f32(ctypes.byref(job), dy.size, None) == A.OK, lib.gnnmp_last_error()
    torch.cuda.synchronize()
    return dz.cpu().numpy()


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU 1: the kernels against float64
# ------------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("hid,name,with_f", EDGE_CASES)
def test_edge_kernel_against_float64(lib, graph, hid, name, with_f):
    """hid = 1, 3: 4-byte lanes; 6: 8-byte lanes; 8, 64: 16-byte lanes; 260: a second feature tile with one active lane.  q, z0, a0 within
    1e-5, norm-wise, of float64; without z0 the other two have the same bits"""
    g, s, t = graph
    case = R.edge_case(hid, name, with_f)
    got = run_edge(lib, g, case, name)
    ref = R.edge_ref(s, t, *case, name)
    for what, a, b in zip(("q", "z0", "a0"), got, ref):
        close(a, b, what)
    assert not got[0][R.q_zero(s, t)].any()
    again = run_edge(lib, g, case, name, want_z0=False)
    assert again[1] is None and np.array_equal(bits(again[0]), bits(got[0])) and np.array_equal(bits(again[2]), bits(got[2]))


@gpu
@pytest.mark.parametrize("Dx", R.DXS)
def test_coordinate_kernels_against_float64(lib, graph, Dx):
    """Dx = 1, 2, 3, 4: exact register capacities; 7 in the capacity of 8, 16 the largest.  x' of K2, dmx and dx of K3 within 1e-5 of
    float64; K3 three ways — dmx only, dx only, both — with equal bits; rows without in-edges keep x_i, bit for bit; the self loop and
    the coincident pair give finite values: dmx = 0 there, and dx equals the reference's (the q = 0 convention)"""
    g, s, t = graph
    n = R.N_NODES
    x, dxo, mx, dq = R.coord_case(Dx)
    xo = run_coord(lib, g, x, mx)
    close(xo, R.coord_ref(s, t, n, x, mx), "x'")
    indeg = np.bincount(t, minlength=n)
    assert (indeg == 0).sum() >= 1 and np.array_equal(bits(xo[indeg == 0]), bits(x[indeg == 0]))
    dmx_ref, dx_ref = R.coord_grad_ref(s, t, n, x, dxo, mx, dq)
    both = run_coord_grad(lib, g, x, dxo, mx, dq, True, True)
    close(both[0], dmx_ref, "dmx")
    close(both[1], dx_ref, "dx")
    assert not both[0][R.q_zero(s, t)].any()
    only_dmx = run_coord_grad(lib, g, x, dxo, mx, dq, True, False)
    only_dx = run_coord_grad(lib, g, x, dxo, mx, dq, False, True)
    assert only_dmx[1] is None and only_dx[0] is None
    assert np.array_equal(bits(only_dmx[0]), bits(both[0])) and np.array_equal(bits(only_dx[1]), bits(both[1]))
    # the three q = 0 edges alone, on their own nodes: dx there is finite and the reference's
    for node in (R.SELF, R.COIN_A, R.COIN_B):
        assert np.all(np.isfinite(both[1][node])) and np.abs(both[1][node] - dx_ref[node]).max() <= 1e-5 * np.abs(dx_ref).max()


@gpu
@pytest.mark.parametrize("name", R.ACTS)
@pytest.mark.parametrize("n", R.ACT_NS)
def test_act_grad_z_against_float64(lib, n, name):
    """n = 1, 5: the element-wise tail alone; 4099: 16-byte lanes and a tail of three"""
    dy, z = R.act_case(n, name)
    close(run_act_z(lib, dy, z, name), R.act_grad_z_ref(dy, z, name), f"dz {name}")


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU 2: the layer
# ------------------------------------------------------------------------------------------------------------------------------------
def make_layer(shape, residual, pe, px, ph):
    import gnnmp
    nin, ein, out, hid = shape
    l = gnnmp.EGNNConv(((nin, ein), out), hidden_size=hid, residual=residual)
    chain = lambda ch: [(dev(W), None if b is None else dev(b), a) for W, b, a in ch]      # noqa: E731
    l.phi_e, l.phi_x, l.phi_h = chain(pe), chain(px), chain(ph)
    return l


def params(l):
    """{name: tensor} in the naming of egnn_conv_ref.flat"""
    out = {}
    for name in ("phi_e", "phi_x", "phi_h"):
        for k, (W, b, _) in enumerate(getattr(l, name)):
            out[f"dW {name}[{k}]"] = W
            if b is not None:
                out[f"db {name}[{k}]"] = b
    return out


def layer_grads(l, g, h, x, e, dhn, dxo, off=()):
    """dict(hn, xo, dh, dx, de, dW ..., db ...) of egnn_conv_ad as numpy arrays; the leaves named in `off` do not require a gradient"""
    import torch
    import gnnmp
    leaves = dict(dh=dev(h), dx=dev(x), **params(l))
    if e is not None:
        leaves["de"] = dev(e)
    for k, v in leaves.items():
        v.requires_grad_(k not in off)
        v.grad = None
    hn, xo = gnnmp.egnn_conv_ad(l, g, leaves["dh"], leaves["dx"], leaves.get("de"))
    torch.autograd.backward([hn, xo], [dev(dhn), dev(dxo)])
    torch.cuda.synchronize()
    out = dict(hn=hn.detach().cpu().numpy(), xo=xo.detach().cpu().numpy())
    out.update({k: None if v.grad is None else v.grad.cpu().numpy() for k, v in leaves.items()})
    return out


@gpu
@pytest.mark.parametrize("shape,residual", R.LAYER_CASES)
def test_layer_against_the_reference(graph, oracle, shape, residual):
    """egnn_conv_ad(...) and its backward: h', x', dh, dx, de and every dW, db within 1e-5 of float64; h' and x' also within 1e-5 of
    oracle.more_layers.egnn_conv and of gnnmp.egnn_conv; under no_grad the same forward, nothing requiring a gradient"""
    import torch
    import gnnmp
    from oracle import more_layers as ML
    g, s, t = graph
    case = R.layer_case(shape)
    h, x, e, pe, px, ph, dhn, dxo = case
    l = make_layer(shape, residual, pe, px, ph)
    got = layer_grads(l, g, h, x, e, dhn, dxo)
    _, ref = R.layer64(s, t, R.N_NODES, case, residual)
    assert set(ref) == set(got)
    for k in ref:
        close(got[k], ref[k], k)
    oh, ox = ML.egnn_conv(s + 1, t + 1, R.N_NODES, h, x, e, pe, px, ph, residual)
    close(got["hn"], oh, "h' against the oracle")
    close(got["xo"], ox, "x' against the oracle")
    with torch.no_grad():
        for p in params(l).values():
            p.requires_grad_(False)
        ed = None if e is None else dev(e)
        ph_, px_ = gnnmp.egnn_conv(l, g, dev(h), dev(x), ed)
        nh, nx = gnnmp.egnn_conv_ad(l, g, dev(h), dev(x), ed)
    close(got["hn"], ph_.cpu().numpy(), "h' against gnnmp.egnn_conv")
    close(got["xo"], px_.cpu().numpy(), "x' against gnnmp.egnn_conv")
    assert not nh.requires_grad and not nx.requires_grad
    assert np.array_equal(bits(nh.cpu().numpy()), bits(got["hn"])) and np.array_equal(bits(nx.cpu().numpy()), bits(got["xo"]))


@gpu
def test_what_needs_no_gradient_gets_none(graph):
    """requires_grad=False on a parameter or an input: its .grad stays None; the others are still within 1e-5 of the reference"""
    import gnnmp
    g, s, t = graph
    shape = (6, 3, 5, 12)
    case = R.layer_case(shape)
    h, x, e, pe, px, ph, dhn, dxo = case
    _, ref = R.layer64(s, t, R.N_NODES, case, False)
    names = [k for k in ref if k not in ("hn", "xo")]
    pe_names = [k for k in names if "phi_e" in k]
    subsets = (("dx",), ("dh",), ("de",), ("dh", "dx", "de"), tuple(pe_names) + ("dh", "de", "dx"),
               tuple(k for k in names if "phi_h" not in k), ("dW phi_e[0]", "db phi_x[0]", "dW phi_h[1]"), tuple(names))
    for off in subsets:
        l = make_layer(shape, False, pe, px, ph)
        if len(off) == len(names):
            for p in params(l).values():
                p.requires_grad_(False)
            hn, xo = gnnmp.egnn_conv_ad(l, g, dev(h), dev(x), dev(e))
            assert not hn.requires_grad and not xo.requires_grad
            continue
        got = layer_grads(l, g, h, x, e, dhn, dxo, off=off)
        for k in names:
            if k in off:
                assert got[k] is None, (off, k)
            else:
                close(got[k], ref[k], f"{k} without {off}")


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU 3: the memory contract and graph capture, export by export
# ------------------------------------------------------------------------------------------------------------------------------------
def contract_graph():
    s, t = R.graph()
    return A.Graph("egnn", s + 1, t + 1, R.N_NODES)


class Spec:
    """one call of one export on a slab: its arrays, the call, the float64 expectations, and the inputs by name (for reloads)"""

    def __init__(self, arrs, call, want, inputs):
        self.arrs, self.call, self.want, self.inputs = arrs, call, want, inputs


def spec_edge(lib, hid, name, with_f, want_z0, seed=0):
    from gnnmp import _lib
    s, t = R.graph()
    x, Pm, Q, F, c = R.edge_case(hid, name, with_f, seed)
    E = len(s)
    inputs = dict(s=s, t=t, x=x, P=Pm, Q=Q, c=c, **({"F": F} if with_f else {}))
    arrs = [A.Arr(k, "in", v) for k, v in inputs.items()] + [A.Arr("q", "out", shape=(E,)), A.Arr("a0", "out", shape=(E, hid))]
    arrs += [A.Arr("z0", "out", shape=(E, hid))] if want_z0 else []

    def call(slab, stream):
        p = lambda nm: slab.ptr(nm) if nm in slab.arrs else None      # noqa: E731
        job = _lib.EgnnEdgeJob(p("s"), p("t"), 8, 0, p("x"), p("P"), p("Q"), p("F"), p("c"), p("q"), p("a0"), p("z0"), R.ACT_CODE[name])
        return lib.gnnmp_egnn_edge_f32(ctypes.byref(job), E, hid, 3, stream)
    q, z0, a0 = R.edge_ref(s, t, x, Pm, Q, F, c, name)
    want = dict(q=A.E(q), a0=A.E(a0), **({"z0": A.E(z0)} if want_z0 else {}))
    return Spec(arrs, call, want, inputs)


def spec_coord(lib, plans, g, Dx, seed=0):
    from gnnmp import _lib
    s, t = R.graph()
    x, _, mx, _ = R.coord_case(Dx, seed)
    inputs = dict(x=x, mx=mx)
    arrs = [A.Arr(k, "in", v) for k, v in inputs.items()] + [A.Arr("xo", "out", shape=x.shape)]

    def call(slab, stream):
        job = _lib.EgnnCoordJob(slab.ptr("x"), slab.ptr("mx"), slab.ptr("xo"))
        return lib.gnnmp_egnn_coord_f32(plans.get(A.Pl(g)), ctypes.byref(job), Dx, stream)
    return Spec(arrs, call, dict(xo=A.E(R.coord_ref(s, t, R.N_NODES, x, mx))), inputs)


def spec_coord_grad(lib, plans, g, Dx, want_dmx, want_dx, seed=0):
    from gnnmp import _lib
    s, t = R.graph()
    x, dxo, mx, dq = R.coord_case(Dx, seed)
    inputs = dict(x=x, dxo=dxo, **(dict(mx=mx, dq=dq) if want_dx else {}))
    arrs = [A.Arr(k, "in", v) for k, v in inputs.items()]
    arrs += ([A.Arr("dmx", "out", shape=(len(s),))] if want_dmx else []) + ([A.Arr("dx", "out", shape=x.shape)] if want_dx else [])

    def call(slab, stream):
        p = lambda nm: slab.ptr(nm) if nm in slab.arrs else None      # noqa: E731
        job = _lib.EgnnCoordGradJob(p("x"), p("dxo"), p("mx"), p("dq"), p("dmx"), p("dx"))
        plan_t = plans.get(A.Pl(g, T=True)) if want_dx else None
        return lib.gnnmp_egnn_coord_grad_f32(plans.get(A.Pl(g)), plan_t, ctypes.byref(job), Dx, stream)
    dmx, dx = R.coord_grad_ref(s, t, R.N_NODES, x, dxo, mx, dq)
    want = dict(**({"dmx": A.E(dmx)} if want_dmx else {}), **({"dx": A.E(dx)} if want_dx else {}))
    return Spec(arrs, call, want, inputs)


def spec_act_z(lib, n, name, seed=0):
    from gnnmp import _lib
    dy, z = R.act_case(n, name, seed)
    inputs = dict(dy=dy, z=z)
    arrs = [A.Arr(k, "in", v) for k, v in inputs.items()] + [A.Arr("dz", "out", shape=(n,))]

    def call(slab, stream):
        job = _lib.ActGradZJob(slab.ptr("dy"), slab.ptr("z"), slab.ptr("dz"), R.ACT_CODE[name])
        return lib.gnnmp_act_grad_z_f32(ctypes.byref(job), n, stream)
    return Spec(arrs, call, dict(dz=A.E(R.act_grad_z_ref(dy, z, name))), inputs)


def contract_runs(spec):
    """no shift, then each array in turn at 16-, 8- and 4-byte alignment (a shift smaller than the element is skipped for that array)"""
    runs = [{}]
    for a in spec.arrs:
        runs += [{a.name: A.SHIFTS[k]} for k in ("a16", "a8", "a4") if A.SHIFTS[k] % a.dtype.itemsize == 0]
    return runs


def check_contract(lib, make_spec, stream):
    """every output element written and nothing else, under every shift of contract_runs, on a side stream"""
    import torch
    sp = ctypes.c_void_p(stream.cuda_stream)
    for shifts in contract_runs(make_spec()):
        spec = make_spec()
        slab = A.Slab(spec.arrs, "cuda", shifts)
        torch.cuda.synchronize()
        rc = spec.call(slab, sp)
        torch.cuda.synchronize()
        assert rc == A.OK, (shifts, lib.gnnmp_last_error())
        problems = slab.check(spec.want)
        assert not problems, (shifts, problems)


@gpu
@pytest.mark.parametrize("hid,with_f,want_z0", [(8, True, True), (8, False, True), (8, True, False), (6, True, True), (6, False, False)])
def test_memory_contract_of_the_edge_kernel(lib, hid, with_f, want_z0):
    """hid = 8: 16-byte lanes narrow to 8 and 4 under the shifts; hid = 6: 8-byte lanes narrow to 4.  With and without F and z0"""
    import torch
    side = torch.cuda.Stream()
    for k, name in enumerate(("swish", "relu")):
        check_contract(lib, lambda: spec_edge(lib, hid, name, with_f, want_z0, seed=k), side)


@gpu
@pytest.mark.parametrize("Dx", [3, 4, 7])
def test_memory_contract_of_the_coordinate_kernels(lib, Dx):
    """x' of K2; dmx and dx of K3 — both, dmx alone (no plan_t, mx, dq), dx alone — hub rows included"""
    import torch
    side = torch.cuda.Stream()
    plans = A.Plans(lib)
    g = contract_graph()
    try:
        check_contract(lib, lambda: spec_coord(lib, plans, g, Dx), side)
        for want_dmx, want_dx in ((True, True), (True, False), (False, True)):
            check_contract(lib, lambda: spec_coord_grad(lib, plans, g, Dx, want_dmx, want_dx), side)
    finally:
        plans.close()


@gpu
@pytest.mark.parametrize("n", R.ACT_NS)
def test_memory_contract_of_act_grad_z(lib, n):
    import torch
    side = torch.cuda.Stream()
    for name in R.ACTS:
        check_contract(lib, lambda: spec_act_z(lib, n, name), side)


def check_capture(lib, specs):
    """specs: the same call on two sets of values.  Recorded first (capture_error_mode = thread_local: a host wait or an allocation
    would be an error; the outputs still hold poison after the capture), then replayed twice with new values in the same buffers: each
    replay is bit-equal to an eager call on the same values, made afterwards"""
    import torch
    side = torch.cuda.Stream()
    sp = ctypes.c_void_p(side.cuda_stream)
    slab = A.Slab(specs[0].arrs)
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        graph.capture_begin(capture_error_mode="thread_local")
        try:
            rc = specs[0].call(slab, sp)
        finally:
            graph.capture_end()
    torch.cuda.synchronize()
    assert rc == A.OK, lib.gnnmp_last_error()
    assert not slab.check({}, untouched=True), "work ran while the call was being recorded"
    replayed = []
    for spec in specs:
        slab.reload(spec.inputs)
        graph.replay()
        torch.cuda.synchronize()
        assert not slab.check(spec.want)
        replayed.append(slab.outputs())
    assert any(not np.array_equal(replayed[0][k], replayed[1][k]) for k in replayed[0])
    for spec, rep in zip(specs, replayed):
        slab.reload(spec.inputs)
        torch.cuda.synchronize()
        assert spec.call(slab, sp) == A.OK, lib.gnnmp_last_error()
        torch.cuda.synchronize()
        eager = slab.outputs()
        assert all(np.array_equal(eager[k], rep[k]) for k in eager)
    del graph


@gpu
def test_the_exports_record_into_a_hip_graph_without_an_eager_call(lib):
    plans = A.Plans(lib)      # new plans, built before the recording (a plan build synchronises): nothing has run on them
    g = contract_graph()
    try:
        plans.get(A.Pl(g)), plans.get(A.Pl(g, T=True))
        check_capture(lib, [spec_edge(lib, 8, "swish", True, True, seed=sd) for sd in (100, 101)])
        check_capture(lib, [spec_coord(lib, plans, g, 3, seed=sd) for sd in (100, 101)])
        check_capture(lib, [spec_coord_grad(lib, plans, g, 3, True, True, seed=sd) for sd in (100, 101)])
        check_capture(lib, [spec_act_z(lib, 4099, "swish", seed=sd) for sd in (100, 101)])
    finally:
        plans.close()


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU 4: determinism, empty graphs
# ------------------------------------------------------------------------------------------------------------------------------------
@gpu
def test_two_calls_give_equal_bits(lib, graph):
    g, _, _ = graph
    same = lambda a, b: all(np.array_equal(bits(u), bits(v)) for u, v in zip(a, b))      # noqa: E731
    for hid, name in ((64, "swish"), (6, "tanh"), (3, "softplus")):
        case = R.edge_case(hid, name, True)
        assert same(run_edge(lib, g, case, name), run_edge(lib, g, case, name)), (hid, name)
    for Dx in (3, 16):
        x, dxo, mx, dq = R.coord_case(Dx)
        assert same([run_coord(lib, g, x, mx)], [run_coord(lib, g, x, mx)])
        assert same(run_coord_grad(lib, g, x, dxo, mx, dq, True, True), run_coord_grad(lib, g, x, dxo, mx, dq, True, True))
    dy, z = R.act_case(4099, "swish")
    assert same([run_act_z(lib, dy, z, "swish")], [run_act_z(lib, dy, z, "swish")])
    shape = (64, 16, 64, 64)
    h, x, e, pe, px, ph, dhn, dxo = R.layer_case(shape)
    l = make_layer(shape, True, pe, px, ph)
    first, again = layer_grads(l, g, h, x, e, dhn, dxo), layer_grads(l, g, h, x, e, dhn, dxo)
    for k in first:
        assert np.array_equal(bits(first[k]), bits(again[k])), k


@gpu
def test_empty_graphs(lib):
    """N = 0 launches nothing (the plan's head says so); E = 0 with N > 0 writes x' = x and dx = Δx', and the layer runs"""
    import torch
    import gnnmp
    none = _FakePlan(n_src=0, n_dst=0, n_edges=0, n_total=0)
    assert _coord(lib, ctypes.addressof(none)) == A.OK and _coord_grad(lib, ctypes.addressof(none), ctypes.addressof(none)) == A.OK
    assert _edge(lib, E=0) == A.OK and _act_z(lib, n=0) == A.OK
    n = 9
    nothing = np.zeros(0, np.int64)
    g = gnnmp.GNNGraph(dev(nothing), dev(nothing), num_nodes=n, index_base=0)
    rng = np.random.default_rng(0)
    x, dxo = [rng.standard_normal((n, 3)).astype(f32) for _ in range(2)]
    one = np.zeros(1, f32)      # E = 0: no entry of mx, dq is read, none of dmx written
    assert np.array_equal(bits(run_coord(lib, g, x, one)), bits(x))
    dmx, dx = run_coord_grad(lib, g, x, dxo, one, one, True, True)
    assert dmx.size == 0 and np.array_equal(bits(dx), bits(dxo))
    # with the edge arrays absent altogether (NULL): a plan without edges reads none of them
    from gnnmp import _lib
    xd, dd, out = dev(x), dev(dxo), nan_like(x.shape)
    job = _lib.EgnnCoordJob(ptr(xd), None, ptr(out))
    assert lib.gnnmp_egnn_coord_f32(g.plan(False).handle, ctypes.byref(job), 3, None) == A.OK, lib.gnnmp_last_error()
    gjob = _lib.EgnnCoordGradJob(ptr(xd), ptr(dd), None, None, None, ptr(out))
    torch.cuda.synchronize()
    assert np.array_equal(bits(out.cpu().numpy()), bits(x))
    assert lib.gnnmp_egnn_coord_grad_f32(g.plan(False).handle, g.plan_transposed(False).handle, ctypes.byref(gjob), 3, None) == A.OK
    torch.cuda.synchronize()
    assert np.array_equal(bits(out.cpu().numpy()), bits(dxo))


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU 5: what egnn_conv_ad refuses
# ------------------------------------------------------------------------------------------------------------------------------------
@gpu
def test_egnn_conv_ad_refuses_by_name(graph):
    import gnnmp
    g, _, _ = graph
    shape = (6, 3, 5, 12)
    h, x, e, pe, px, ph, _, _ = R.layer_case(shape)
    l = make_layer(shape, False, pe, px, ph)
    ht, xt, et = dev(h), dev(x), dev(e)
    with pytest.raises(NotImplementedError, match="bipartite"):
        gnnmp.egnn_conv_ad(l, g, (ht, ht), xt, et)
    with pytest.raises(ValueError, match="Dx > 16"):
        gnnmp.egnn_conv_ad(l, g, ht, dev(np.zeros((R.N_NODES, 17), f32)), et)
    with pytest.raises(ValueError, match="e has 2 features, the layer was built for 3"):
        gnnmp.egnn_conv_ad(l, g, ht, xt, et[:, :2].contiguous())
    with pytest.raises(ValueError, match="built with edge features"):
        gnnmp.egnn_conv_ad(l, g, ht, xt)
    plain = make_layer((6, 0, 5, 12), False, [(pe[0][0][:, :13].copy(),) + pe[0][1:], pe[1]], px, ph)
    with pytest.raises(ValueError, match="built without edge features"):
        gnnmp.egnn_conv_ad(plain, g, ht, xt, et)
    wide = make_layer(shape, False, pe, [px[0], (np.concatenate([px[1][0]] * 2),) + px[1][1:]], ph)
    with pytest.raises(ValueError, match="last ϕx layer has 2 outputs"):
        gnnmp.egnn_conv_ad(wide, g, ht, xt, et)
    short = make_layer(shape, False, [(pe[0][0][:, :-1].copy(),) + pe[0][1:], pe[1]], px, ph)
    with pytest.raises(ValueError, match="first ϕe weight has 15 columns"):
        gnnmp.egnn_conv_ad(short, g, ht, xt, et)
    narrow = make_layer(shape, False, pe, px, [(ph[0][0][:, :-2].copy(),) + ph[0][1:], ph[1]])
    with pytest.raises(ValueError, match="first ϕh weight has 16 columns"):
        gnnmp.egnn_conv_ad(narrow, g, ht, xt, et)


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU 6: a small EGNN step
# ------------------------------------------------------------------------------------------------------------------------------------
@gpu
def test_a_small_egnn_step():
    """radius_graph(pos) -> two EGNNConv((16, 0) => 16, residual), the second on the coordinates the first one moved -> global_pool_ad
    mean; 4 clouds of 48 points on jittered lattices, loss = Σ pooled .* R + Σ x2 .* Rx, so the coordinate gradient flows through both
    layers: all parameter gradients, dh and dpos against the float64 chain on the edge list the device built.  The radius gives every
    cloud a mean degree of at least 4, no node more than 12 neighbours, and every node at least one."""
    import torch
    import gnnmp
    from gnnmp.backward import global_pool_ad
    pos, gi, h, layers, Rm, Rx = R.step_case()
    c = R.STEP
    n = len(pos)
    pd = dev(pos).requires_grad_(True)
    g = gnnmp.radius_graph(pd.detach(), c["radius"], graph_indicator=dev(gi + 1))
    s, t = g.s.cpu().numpy() - 1, g.t.cpu().numpy() - 1
    assert np.array_equal(gi[s], gi[t]) and not (s == t).any()
    deg = np.bincount(t, minlength=n)
    per_cloud = deg.reshape(c["clouds"], c["pts"]).mean(axis=1)
    print(f"radius graph: {len(s)} edges, mean degree per cloud {per_cloud}, min {deg.min()}, max {deg.max()}")
    assert per_cloud.min() >= 4 and deg.max() <= 12 and deg.min() >= 1
    ls = [make_layer((c["nin"], 0, c["nin"], 2 * c["nin"]), True, *w) for w in layers]
    for l in ls:
        for p in params(l).values():
            p.requires_grad_(True)
    ht = dev(h).requires_grad_(True)
    h1, x1 = gnnmp.egnn_conv_ad(ls[0], g, ht, pd)
    h2, x2 = gnnmp.egnn_conv_ad(ls[1], g, h1, x1)
    pooled = global_pool_ad(gnnmp.GlobalPool("mean"), g, h2)
    ((pooled * dev(Rm)).sum() + (x2 * dev(Rx)).sum()).backward()
    torch.cuda.synchronize()
    h2_ref, x2_ref, grads, dh_ref, dpos_ref = R.step_grad64(s, t, gi, h, pos, layers, Rm, Rx)
    close(h2.detach().cpu().numpy(), h2_ref, "h2")
    close(x2.detach().cpu().numpy(), x2_ref, "x2")
    for i, (l, bw) in enumerate(zip(ls, grads)):
        ref = R.flat(dict(hn=None, xo=None), bw)
        for k, p in params(l).items():
            close(p.grad.cpu().numpy(), ref[k], f"{k} of layer {i + 1}")
    close(ht.grad.cpu().numpy(), dh_ref, "dh")
    close(pd.grad.cpu().numpy(), dpos_ref, "dpos")
