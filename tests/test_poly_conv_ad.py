"""cheb_conv_ad, d_conv_ad and the two exports of csrc/poly_conv.hip: gnnmp_poly_hop_f32 and gnnmp_gru_pointwise_grad_f32 (include/gnnmp.h
states the arithmetic; the gated layers that use the GRU pullback are in tests/test_gated_conv_ad.py).

Without a GPU: the two exports exist in header, SYMBOLS and library and take const plans and const host records whose ctypes mirrors have
the header's layout; every refusal of the header comes before any HIP call; N = 0 returns OK; the float64 models (tests/poly_conv_ref.py)
agree with central finite differences in every argument and with oracle.more_layers.cheb_conv / d_conv; the operands of every GPU case keep
the float32 restatement of the header's formulas within 2e-6 of float64.

On the GPU: the hop within 1e-5 of float64, norm-wise and element-wise, over the plan and the transposed plan of the 40-node multigraph
(self loops, a repeated edge, a node without in-edges, one without out-edges, a hub of 600 edges in and 600 out), at every lane width, tail
and tile count, for all 64 combinations of optional operands; the bits of gnnmp_propagate_slots_f32 for alpha = 1 alone; out aliasing prev
and add; every output element written and nothing else at any pointer alignment; equal bits of two calls; recorded into a HIP graph without
an eager call.  The GRU pullback likewise.  The two layers: forward against float64 and the existing forward, every gradient (dx at 1e-5;
weights and biases inside γ_n Σ|terms|, n as tests/poly_conv_ref.py: sum_n reasons), pruning, refusals."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_cases as A  # noqa: E402
import gated_conv_ref as G  # noqa: E402
import poly_conv_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOP, GRU = "gnnmp_poly_hop_f32", "gnnmp_gru_pointwise_grad_f32"
gpu = pytest.mark.gpu
f32, f64 = np.float32, np.float64
RECORDS = {HOP: ("gnnmp_poly_hop_t", "PolyHopJob", ("z", "w_slot", "ss_slot", "scale_dst", "self", "prev", "add", "alpha", "beta", "gamma", "out")),
           GRU: ("gnnmp_gru_grad_t", "GruGradJob", ("gx", "gh", "b", "h", "dout", "base", "dgx", "dgh", "dh"))}
PARAMS = {HOP: ["plan", "job", "D", "stream"], GRU: ["job", "N", "D", "stream"]}


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
    for name in (HOP, GRU):
        assert f"int {name}(" in header and header.index(f"int {name}(") < internal, name
        assert name in _lib.SYMBOLS and name in exported, name
        assert "} " + RECORDS[name][0] + ";" in header
    for cite in ("GNNlib/src/layers/conv.jl:83-98", "conv.jl:696-724", "conv.jl:218-233"):
        assert cite in header[:internal], cite
    conventions = header[:header.index("#ifndef GNNMP_H")]           # what is capture-tested, and where
    assert HOP in conventions and GRU in conventions and "tests/test_poly_conv_ad.py" in conventions
    for fn in ("cheb_conv_ad", "d_conv_ad", "gated_graph_conv_ad", "res_gated_graph_conv_ad"):
        assert callable(getattr(gnnmp, fn)), fn


@pytest.mark.parametrize("export", [HOP, GRU])
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


def _hop(lib, plan, job=True, z=1, w_slot=2, ss_slot=3, scale_dst=4, self_=5, prev=6, add=7, out=8, alpha=1.0, beta=0.5, gamma=-1.0, D=4):
    from gnnmp import _lib
    j = _lib.PolyHopJob(P_(z), P_(w_slot), P_(ss_slot), P_(scale_dst), P_(self_), P_(prev), P_(add), alpha, beta, gamma, P_(out))
    return lib.gnnmp_poly_hop_f32(plan, ctypes.byref(j) if job else None, D, None)


def _gru(lib, job=True, gx=1, gh=2, b=3, h=4, dout=5, base=6, dgx=7, dgh=8, dh=9, N=5, D=4):
    from gnnmp import _lib
    j = _lib.GruGradJob(P_(gx), P_(gh), P_(b), P_(h), P_(dout), P_(base), P_(dgx), P_(dgh), P_(dh))
    return lib.gnnmp_gru_pointwise_grad_f32(ctypes.byref(j) if job else None, N, D, None)


def test_argument_validation_needs_no_gpu():
    """every refusal of the header comes before the first HIP call: on a machine without a device, on pointers that are not memory"""
    from gnnmp import _lib
    lib = _lib.load()
    EINVAL, err = _lib.EINVAL, lib.gnnmp_last_error
    sq = _FakePlan(n_src=5, n_dst=5, n_edges=7, n_total=7)
    pl = ctypes.addressof(sq)
    assert _hop(lib, None) == EINVAL and b"poly_hop: null plan" in err()
    assert _hop(lib, pl, job=False) == EINVAL and b"poly_hop: null job" in err()
    assert _hop(lib, pl, z=None) == EINVAL and b"poly_hop: null z" in err()
    assert _hop(lib, pl, out=None) == EINVAL and b"poly_hop: null out" in err()
    for D in (0, -1, (1 << 19) + 1, 2 ** 40):
        assert _hop(lib, pl, D=D) == EINVAL and b"poly_hop: bad D" in err(), D
    assert _hop(lib, pl, out=1) == EINVAL and b"out aliases z" in err()
    assert _hop(lib, pl, out=5) == EINVAL and b"out aliases self" in err()
    assert _hop(lib, pl, self_=None) == EINVAL and b"beta != 0 with a null self" in err()
    assert _hop(lib, pl, prev=None) == EINVAL and b"gamma != 0 with a null prev" in err()
    assert _gru(lib, job=False) == EINVAL and b"gru_pointwise_grad: null job" in err()
    assert _gru(lib, N=-1) == EINVAL and b"negative N" in err()
    for D in (0, -3, (1 << 20) + 1):
        assert _gru(lib, D=D) == EINVAL and b"gru_pointwise_grad: bad D" in err(), D
    for name in ("gx", "gh", "h", "dout"):
        assert _gru(lib, **{name: None}) == EINVAL and b"null gx, gh, h or dout" in err(), name
    for name in ("dgx", "dgh", "dh"):
        assert _gru(lib, **{name: None}) == EINVAL and b"null dgx, dgh or dh" in err(), name


def test_empty_sizes_return_ok_without_a_device():
    """n_dst = 0 / N = 0 launch nothing — with and without the optional pointers, on a plan that is not square and one with self loops"""
    from gnnmp import _lib
    lib = _lib.load()
    for plan in (_FakePlan(n_src=0, n_dst=0, n_edges=0, n_total=0), _FakePlan(n_src=9, n_dst=0, n_edges=0, n_total=0)):
        pn = ctypes.addressof(plan)
        assert _hop(lib, pn) == _lib.OK
        assert _hop(lib, pn, w_slot=None, ss_slot=None, scale_dst=None, self_=None, prev=None, add=None, beta=0.0, gamma=0.0, D=1 << 19) == _lib.OK
        assert _hop(lib, pn, out=6) == _lib.OK and _hop(lib, pn, out=7) == _lib.OK      # out = prev, out = add
    assert _gru(lib, N=0) == _lib.OK
    assert _gru(lib, N=0, b=None, base=None, D=1 << 20) == _lib.OK
    assert _gru(lib, N=0, base=9) == _lib.OK                                           # base = dh


# ------------------------------------------------------------------------------------------------------------------------------------
# CPU: the references
# ------------------------------------------------------------------------------------------------------------------------------------
def fd_check(loss, operands, h=1e-6):
    """central differences of `loss()` in every element of every (array, gradient, name)"""
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


@pytest.mark.parametrize("kind", R.CHEB_WEIGHTS)
@pytest.mark.parametrize("k", R.CHEB_KS)
def test_cheb_reference_gradient_agrees_with_finite_differences(k, kind):
    """dx, dW and db of the float64 ChebConv model (Clenshaw over the transposed operator) against central differences, with symmetric and
    asymmetric weights: the transposition is not a no-op"""
    s, t, n = R.bidirected_graph()
    x, W, b, w, dY = [None if a is None else a.astype(f64) for a in R.cheb_case(k, True, kind)]
    lam = R.cheb_lam(kind)
    ref = R.cheb_grad(s, t, n, x, W, b, lam, dY, w)
    fd_check(lambda: float((R.cheb_forward(s, t, n, x, W, b, lam, w) * dY).sum()), [(x, ref["dx"], "dx"), (W, ref["dW"], "dW"), (b, ref["db"], "db")])


@pytest.mark.parametrize("k,weighted", R.DCONV_CASES)
def test_dconv_reference_gradient_agrees_with_finite_differences(k, weighted):
    s, t, n = R.directed_graph()
    x, W, b, w, dY = [None if a is None else a.astype(f64) for a in R.dconv_case(k, weighted)]
    ref = R.dconv_grad(s, t, n, x, W, b, dY, w)
    fd_check(lambda: float((R.dconv_forward(s, t, n, x, W, b, w) * dY).sum()), [(x, ref["dx"], "dx"), (W, ref["dW"], "dW"), (b, ref["db"], "db")])


def _close64(got, ref, tol=1e-5):
    got, ref = np.asarray(got, f64), np.asarray(ref, f64)
    return np.linalg.norm(got - ref) <= tol * np.linalg.norm(ref) and np.abs(got - ref).max() <= tol * np.abs(ref).max()


@pytest.mark.parametrize("k,bias,kind", R.CHEB_CASES)
def test_cheb_reference_forward_agrees_with_the_oracle(k, bias, kind):
    """the float64 model against oracle.more_layers.cheb_conv (float32 numpy on the dense L̃, 1-based indices) at 1e-5, λmax as the oracle
    takes it"""
    from oracle import more_layers as ML
    s, t, n = R.bidirected_graph()
    x, W, b, w, _ = R.cheb_case(k, bias, kind)
    ref = R.cheb_ref(k, bias, kind, R.cheb_lam(kind))
    assert _close64(ML.cheb_conv(s + 1, t + 1, n, x, W, b, k, edge_weight=w), ref["Y"])


@pytest.mark.parametrize("k,weighted", R.DCONV_CASES)
def test_dconv_reference_forward_agrees_with_the_oracle(k, weighted):
    from oracle import more_layers as ML
    s, t, n = R.directed_graph()
    x, W, b, w, _ = R.dconv_case(k, weighted)
    assert _close64(ML.d_conv(s + 1, t + 1, n, x, W, b, k, edge_weight=w), R.dconv_ref(k, weighted)["Y"])


@pytest.mark.parametrize("transposed", [False, True], ids=["plan", "plan_t"])
@pytest.mark.parametrize("D", R.WIDTHS)
def test_the_hop_cases_are_well_conditioned(D, transposed):
    """THE CONDITION ON THE INPUTS, not a measurement: the header's formula in float32 is within 2e-6, norm-wise, of float64 for every
    combination of optional operands"""
    worst = R.hop_condition(D, transposed)
    assert worst <= R.COND, f"the float32 restatement is {worst:.2e} from float64 (bound {R.COND:g})"


@pytest.mark.parametrize("D", G.GRU_DS)
def test_the_gru_cases_are_well_conditioned(D):
    for with_b in (True, False):
        for with_base in (True, False):
            assert G.gru_condition(D, with_b, with_base) <= G.COND


@pytest.mark.parametrize("k,bias,kind", R.CHEB_CASES)
def test_the_cheb_cases_are_well_conditioned(k, bias, kind):
    assert R.cheb_condition(k, bias, kind, R.cheb_lam(kind)) <= R.COND


@pytest.mark.parametrize("k,weighted", R.DCONV_CASES)
def test_the_dconv_cases_are_well_conditioned(k, weighted):
    """DConv multiplies by the raw degree at every step: the graph keeps the degrees small and k <= 3"""
    assert R.dconv_condition(k, weighted) <= R.COND


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


def within_sum_bound(got, ref, mag, n, what):
    """|got − ref64| <= γ_n Σ|terms|, element-wise"""
    got, ref = np.asarray(got, f64), np.asarray(ref, f64)
    assert got.shape == ref.shape and np.all(np.isfinite(got)), what
    bound = R.gamma(n) * mag
    used = float((np.abs(got - ref) / np.maximum(bound, 1e-300)).max()) if got.size else 0.0
    print(f"{what}: uses {used:.3f} of the summation bound (n = {n})")
    assert np.all(np.abs(got - ref) <= bound), f"{what}: {used:.2f} of the summation bound"
    return used


def ptr(v):
    return None if v is None else ctypes.c_void_p(v.data_ptr())


def call_hop(lib, plan, p, alpha, beta, gamma, D, stream=None, out="out"):
    """p(name) -> pointer | None for z, w_slot, ss_slot, scale_dst, self, prev, add, out"""
    from gnnmp import _lib
    job = _lib.PolyHopJob(p("z"), p("w_slot"), p("ss_slot"), p("scale_dst"), p("self"), p("prev"), p("add"), alpha, beta, gamma, p(out))
    return lib.gnnmp_poly_hop_f32(plan, ctypes.byref(job), D, stream)


def call_gru(lib, p, N, D, stream=None, dh="dh"):
    from gnnmp import _lib
    job = _lib.GruGradJob(p("gx"), p("gh"), p("b"), p("h"), p("dout"), p("base"), p("dgx"), p("dgh"), p(dh))
    return lib.gnnmp_gru_pointwise_grad_f32(ctypes.byref(job), N, D, stream)


NAMES = dict(zip(R.FIELDS, ("w_slot", "ss_slot", "scale_dst", "self", "prev", "add")))      # the model's operand -> the record's field


def slot_arrays(s, t, ops, combo):
    """{record field: float32 array} of a hop case: the per-edge factors in the plan's slot order (stable by destination)"""
    order = np.argsort(t, kind="stable")
    arrs = {"z": ops["z"]}
    for k, on in zip(R.FIELDS, combo):
        if on:
            arrs[NAMES[k]] = ops[k][order] if k in ("w", "ss") else ops[k]
    return arrs


def coeffs(combo):
    on = dict(zip(R.FIELDS, combo))
    return R.ALPHA, R.BETA if on["self_"] else 0.0, R.GAMMA if on["prev"] else 0.0


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
    return g


def nan(*shape):
    import torch
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU 1: the hop
# ------------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("transposed", [False, True], ids=["plan", "plan_t"])
@pytest.mark.parametrize("D", R.WIDTHS)
def test_hop_against_float64(lib, graph, D, transposed):
    """D = 1, 3, 7: 4-byte lanes; 2, 6: 8-byte lanes; 64, 100, 260: 16-byte lanes (100: 25 of 32 lanes active; 260: a second feature tile
    with one active lane).  All 64 combinations of w_slot, ss_slot, scale_dst, self, prev, add present or NULL within 1e-5 of float64;
    the row without slots gets the epilogue of a zero aggregate; equal bits of two calls"""
    import torch
    s, t, ops = R.hop_case(D, transposed)
    plan = (graph.plan_transposed(False) if transposed else graph.plan(False)).handle
    empty = R.NO_OUT if transposed else R.NO_IN
    for combo in R.COMBOS:
        held = {k: dev(v) for k, v in slot_arrays(s, t, ops, combo).items()}
        out = held["out"] = nan(R.N_NODES, D)
        a, b, c = coeffs(combo)
        rc = call_hop(lib, plan, lambda nm: ptr(held.get(nm)), a, b, c, D)
        assert rc == A.OK, lib.gnnmp_last_error()
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        close(got, R.hop_ref(D, transposed, combo), f"hop {combo}")
        on = dict(zip(R.FIELDS, combo))
        want0 = np.zeros(D, f32)
        want0 = want0 + f32(b) * ops["self_"][empty] if on["self_"] else want0
        want0 = want0 + f32(c) * ops["prev"][empty] if on["prev"] else want0
        want0 = want0 + ops["add"][empty] if on["add"] else want0
        assert np.array_equal(got[empty], want0), "the row without slots is the epilogue of a zero aggregate"
        held["out"] = again = nan(R.N_NODES, D)
        assert call_hop(lib, plan, lambda nm: ptr(held.get(nm)), a, b, c, D) == A.OK
        torch.cuda.synchronize()
        assert np.array_equal(bits(again.cpu().numpy()), bits(got))


@gpu
@pytest.mark.parametrize("D", [1, 6, 64, 100, 260])
def test_hop_alone_has_the_bits_of_propagate_slots(lib, D):
    """alpha = 1 and no other term: gnnmp_propagate_slots_f32's bits on a plan without split rows, for every combination of w_slot, ss_slot
    and scale_dst — the per-slot factor and the fold are the same expressions"""
    import torch
    g = A.random_graph("short", 40, 300, seed=77)
    plans = A.Plans(lib)
    try:
        plan = plans.get(A.Pl(g))
        info = (ctypes.c_int64 * 8)()
        assert lib.gnnmp_plan_info(plan, info) == A.OK and info[5] == 0, "the plan splits a row"
        rng = np.random.default_rng([D, 78])
        z = dev(rng.standard_normal((40, D)).astype(f32))
        w, ss = dev(rng.uniform(0.5, 1.5, g.E).astype(f32)), dev(rng.uniform(0.5, 1.5, g.E).astype(f32))
        sd = dev(rng.uniform(0.5, 1.5, 40).astype(f32))
        for mask in range(8):
            held = {"z": z, "w_slot": w if mask & 1 else None, "ss_slot": ss if mask & 2 else None, "scale_dst": sd if mask & 4 else None}
            want, held["out"] = nan(40, D), nan(40, D)
            rc = lib.gnnmp_propagate_slots_f32(plan, 0, ptr(z), ptr(held["w_slot"]), ptr(held["ss_slot"]), ptr(held["scale_dst"]), ptr(want), D, None)
            assert rc == A.OK, lib.gnnmp_last_error()
            assert call_hop(lib, plan, lambda nm: ptr(held.get(nm)), 1.0, 0.0, 0.0, D) == A.OK, lib.gnnmp_last_error()
            torch.cuda.synchronize()
            assert np.array_equal(bits(held["out"].cpu().numpy()), bits(want.cpu().numpy())), mask
    finally:
        plans.close()


@gpu
@pytest.mark.parametrize("transposed", [False, True], ids=["plan", "plan_t"])
@pytest.mark.parametrize("D", [3, 6, 260])
def test_hop_out_may_alias_prev_or_add(lib, graph, D, transposed):
    """out = prev and out = add give the bits of the call with a separate out: each element is read by the lane that writes it"""
    import torch
    s, t, ops = R.hop_case(D, transposed)
    plan = (graph.plan_transposed(False) if transposed else graph.plan(False)).handle
    combo = (True,) * 6
    a, b, c = coeffs(combo)
    held = {k: dev(v) for k, v in slot_arrays(s, t, ops, combo).items()}
    held["out"] = nan(R.N_NODES, D)
    assert call_hop(lib, plan, lambda nm: ptr(held.get(nm)), a, b, c, D) == A.OK
    torch.cuda.synchronize()
    want = held["out"].cpu().numpy()
    for alias in ("prev", "add"):
        fresh = {k: dev(v) for k, v in slot_arrays(s, t, ops, combo).items()}
        assert call_hop(lib, plan, lambda nm: ptr(fresh.get(nm)), a, b, c, D, out=alias) == A.OK, lib.gnnmp_last_error()
        torch.cuda.synchronize()
        assert np.array_equal(bits(fresh[alias].cpu().numpy()), bits(want)), alias


def contract_graph():
    s, t, _ = R.graph()
    return A.Graph("poly", s + 1, t + 1, R.N_NODES)


def hop_arrays(D, transposed, combo, seed=0):
    s, t, ops = R.hop_case(D, transposed, seed)
    return [A.Arr(k, "in", v) for k, v in slot_arrays(s, t, ops, combo).items()] + [A.Arr("out", "out", shape=(R.N_NODES, D))]


def _p(slab):
    return lambda nm: slab.ptr(nm) if nm in slab.arrs else None


@gpu
@pytest.mark.parametrize("transposed", [False, True], ids=["plan", "plan_t"])
@pytest.mark.parametrize("D", [8, 6, 260])
def test_memory_contract_of_the_hop(lib, D, transposed):
    """every element of out written — the row without slots included — no store before or after an array or into an input, with each
    array in turn shifted to 16-, 8- and 4-byte alignment (D = 8, 260: 16-byte lanes narrow to 8 and 4; D = 6: 8-byte lanes narrow to 4),
    on a side stream, the hub rows included; then with operands left out"""
    import torch
    side = torch.cuda.Stream()
    sp = ctypes.c_void_p(side.cuda_stream)
    plans = A.Plans(lib)
    g = contract_graph()
    try:
        plan = plans.get(A.Pl(g, T=transposed))
        full = (True,) * 6
        names = [a.name for a in hop_arrays(D, transposed, full)]
        runs = [({}, full)] + [({nm: A.SHIFTS[a]}, full) for nm in names for a in ("a16", "a8", "a4")]
        runs += [({"z": 4}, (False,) * 6), ({}, (True, False, True, False, True, False)), ({"out": 8}, (False, True, False, True, False, True))]
        for shifts, combo in runs:
            slab = A.Slab(hop_arrays(D, transposed, combo), "cuda", shifts)
            a, b, c = coeffs(combo)
            torch.cuda.synchronize()
            rc = call_hop(lib, plan, _p(slab), a, b, c, D, sp)
            torch.cuda.synchronize()
            assert rc == A.OK, (shifts, lib.gnnmp_last_error())
            problems = slab.check({"out": A.E(R.hop_ref(D, transposed, combo))})
            assert not problems, (shifts, combo, problems)
    finally:
        plans.close()


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
@pytest.mark.parametrize("transposed", [False, True], ids=["plan", "plan_t"])
def test_the_hop_records_into_a_hip_graph_without_an_eager_call(lib, transposed):
    D, combo, seeds = 8, (True,) * 6, (100, 101)
    g = contract_graph()
    plans = A.Plans(lib)
    try:
        plan = plans.get(A.Pl(g, T=transposed))
        slab = A.Slab(hop_arrays(D, transposed, combo, seeds[0]))
        a, b, c = coeffs(combo)
        call = lambda sp: call_hop(lib, plan, _p(slab), a, b, c, D, sp)      # noqa: E731
        reloads = [slot_arrays(*R.hop_case(D, transposed, sd), combo) for sd in seeds]
        wants = [{"out": A.E(R.hop_ref(D, transposed, combo, sd))} for sd in seeds]
        assert not np.array_equal(reloads[0]["z"], reloads[1]["z"])
        _capture_and_replay(lib, slab, call, reloads, wants)
    finally:
        plans.close()


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU 2: the GRU pullback
# ------------------------------------------------------------------------------------------------------------------------------------
GRU_IN = ("gx", "gh", "b", "h", "dout", "base")


def gru_arrays(D, with_b=True, with_base=True, seed=0):
    case = dict(zip(GRU_IN, G.gru_case(D, seed)))
    arrs = [A.Arr(k, "in", v) for k, v in case.items() if (k != "b" or with_b) and (k != "base" or with_base)]
    return arrs + [A.Arr("dgx", "out", shape=(G.GRU_N, 3 * D)), A.Arr("dgh", "out", shape=(G.GRU_N, 3 * D)), A.Arr("dh", "out", shape=(G.GRU_N, D))]


def gru_want(D, with_b, with_base, seed=0):
    return {k: A.E(v) for k, v in zip(("dgx", "dgh", "dh"), G.gru_ref(D, with_b, with_base, seed))}


@gpu
@pytest.mark.parametrize("D", G.GRU_DS)
def test_gru_pointwise_grad_against_float64(lib, D):
    """dgx, dgh, dh within 1e-5 of float64 with and without b and base; base aliasing dh gives the bits of the separate call; the gates are
    those of gnnmp_gru_pointwise_f32 (dh without base is Δ z: z recovered exactly where h' was computed from it); equal bits of two calls"""
    import torch
    case = dict(zip(GRU_IN, G.gru_case(D)))
    for with_b in (True, False):
        for with_base in (True, False):
            held = {k: dev(v) for k, v in case.items() if (k != "b" or with_b) and (k != "base" or with_base)}
            runs = []
            for _ in range(2):
                held.update(dgx=nan(G.GRU_N, 3 * D), dgh=nan(G.GRU_N, 3 * D), dh=nan(G.GRU_N, D))
                assert call_gru(lib, lambda nm: ptr(held.get(nm)), G.GRU_N, D) == A.OK, lib.gnnmp_last_error()
                torch.cuda.synchronize()
                runs.append([held[k].cpu().numpy() for k in ("dgx", "dgh", "dh")])
            for got, want, what in zip(runs[0], G.gru_ref(D, with_b, with_base), ("dgx", "dgh", "dh")):
                close(got, want, what)
            assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(*runs))
            if with_base:
                held.update(dgx=nan(G.GRU_N, 3 * D), dgh=nan(G.GRU_N, 3 * D), base=dev(case["base"]))
                assert call_gru(lib, lambda nm: ptr(held.get(nm)), G.GRU_N, D, dh="base") == A.OK, lib.gnnmp_last_error()
                torch.cuda.synchronize()
                for got, want in zip([held[k].cpu().numpy() for k in ("dgx", "dgh", "base")], runs[0]):
                    assert np.array_equal(bits(got), bits(want))


@gpu
@pytest.mark.parametrize("D", [8, 6, 33])
def test_memory_contract_of_the_gru_pullback(lib, D):
    """every element of dgx, dgh, dh written and nothing beyond, with each array in turn at 16-, 8- and 4-byte alignment, on a side stream;
    then without b, without base"""
    import torch
    side = torch.cuda.Stream()
    sp = ctypes.c_void_p(side.cuda_stream)
    names = [a.name for a in gru_arrays(D)]
    runs = [({}, {})] + [({nm: A.SHIFTS[a]}, {}) for nm in names for a in ("a16", "a8", "a4")]
    runs += [({"gx": 4}, dict(with_b=False)), ({"dh": 8}, dict(with_base=False)), ({}, dict(with_b=False, with_base=False))]
    for shifts, opts in runs:
        slab = A.Slab(gru_arrays(D, **opts), "cuda", shifts)
        torch.cuda.synchronize()
        rc = call_gru(lib, _p(slab), G.GRU_N, D, sp)
        torch.cuda.synchronize()
        assert rc == A.OK, (shifts, lib.gnnmp_last_error())
        problems = slab.check(gru_want(D, opts.get("with_b", True), opts.get("with_base", True)))
        assert not problems, (shifts, opts, problems)


@gpu
def test_the_gru_pullback_records_into_a_hip_graph_without_an_eager_call(lib):
    D, seeds = 5, (100, 101)
    slab = A.Slab(gru_arrays(D, seed=seeds[0]))
    call = lambda sp: call_gru(lib, _p(slab), G.GRU_N, D, sp)      # noqa: E731
    reloads = [dict(zip(GRU_IN, G.gru_case(D, sd))) for sd in seeds]
    wants = [gru_want(D, True, True, sd) for sd in seeds]
    _capture_and_replay(lib, slab, call, reloads, wants)


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU 3: the layers
# ------------------------------------------------------------------------------------------------------------------------------------
def cheb_layer(k, bias, kind):
    """(layer, graph, x, dY, λmax of the device path)"""
    import gnnmp
    s, t, n = R.bidirected_graph()
    x, W, b, w, dY = R.cheb_case(k, bias, kind)
    g = gnnmp.GNNGraph(dev(s), dev(t), None if w is None else dev(w), num_nodes=n, index_base=0)
    l = gnnmp.ChebConv((W.shape[2], W.shape[1]), k, bias=bias)
    l.weight = dev(W)
    if bias:
        l.bias = dev(b)
    lam = gnnmp.layers_more.scaled_laplacian_op(g)[3]
    return l, g, x, dY, lam


@gpu
@pytest.mark.parametrize("k,bias,kind", R.CHEB_CASES)
def test_cheb_conv_ad(k, bias, kind):
    """forward within 1e-5 of the float64 model (with the device path's λmax: Lanczos error is not part of this comparison) and of
    gnnmp.cheb_conv; dx within 1e-5; dW, db inside γ_n Σ|terms|; the operands keep the float32 restatement within 2e-6 at that λmax"""
    import torch
    import gnnmp
    l, g, x, dY, lam = cheb_layer(k, bias, kind)
    assert R.cheb_condition(k, bias, kind, lam) <= R.COND
    ref = R.cheb_ref(k, bias, kind, lam)
    with torch.no_grad():
        y0 = gnnmp.cheb_conv_ad(l, g, dev(x))
        plain = gnnmp.cheb_conv(l, g, dev(x))
    close(y0.cpu().numpy(), ref["Y"], "Y")
    close(y0.cpu().numpy(), plain.cpu().numpy(), "Y / cheb_conv")
    xt = dev(x).requires_grad_(True)
    leaves = [l.weight] + ([l.bias] if bias else [])
    for p in leaves:
        p.requires_grad_(True)
        p.grad = None
    y = gnnmp.cheb_conv_ad(l, g, xt)
    assert np.array_equal(bits(y.detach().cpu().numpy()), bits(y0.cpu().numpy()))
    y.backward(dev(dY))
    torch.cuda.synchronize()
    close(xt.grad.cpu().numpy(), ref["dx"], "dx")
    s, t, n = R.bidirected_graph()
    nn = R.sum_n(n, len(s), k)
    within_sum_bound(l.weight.grad.cpu().numpy(), ref["dW"], ref["mag_W"], nn, "dW")
    if bias:
        within_sum_bound(l.bias.grad.cpu().numpy(), ref["db"], ref["mag_b"], nn, "db")


def dconv_layer(k, weighted):
    import gnnmp
    s, t, n = R.directed_graph()
    x, W, b, w, dY = R.dconv_case(k, weighted)
    g = gnnmp.GNNGraph(dev(s), dev(t), None if w is None else dev(w), num_nodes=n, index_base=0)
    l = gnnmp.DConv((W.shape[3], W.shape[2]), k)
    l.weights, l.bias = dev(W), dev(b)
    return l, g, x, dY


@gpu
@pytest.mark.parametrize("k,weighted", R.DCONV_CASES)
def test_d_conv_ad(k, weighted):
    """forward within 1e-5 of the float64 model and of gnnmp.d_conv on a directed graph; dx within 1e-5; dweights, dbias inside γ_n Σ|terms|"""
    import torch
    import gnnmp
    l, g, x, dY = dconv_layer(k, weighted)
    ref = R.dconv_ref(k, weighted)
    with torch.no_grad():
        y0 = gnnmp.d_conv_ad(l, g, dev(x))
        plain = gnnmp.d_conv(l, g, dev(x))
    close(y0.cpu().numpy(), ref["Y"], "Y")
    close(y0.cpu().numpy(), plain.cpu().numpy(), "Y / d_conv")
    xt = dev(x).requires_grad_(True)
    for p in (l.weights, l.bias):
        p.requires_grad_(True)
        p.grad = None
    y = gnnmp.d_conv_ad(l, g, xt)
    assert np.array_equal(bits(y.detach().cpu().numpy()), bits(y0.cpu().numpy()))
    y.backward(dev(dY))
    torch.cuda.synchronize()
    close(xt.grad.cpu().numpy(), ref["dx"], "dx")
    s, t, n = R.directed_graph()
    nn = R.sum_n(n, len(s), k)
    within_sum_bound(l.weights.grad.cpu().numpy(), ref["dW"], ref["mag_W"], nn, "dweights")
    within_sum_bound(l.bias.grad.cpu().numpy(), ref["db"], ref["mag_b"], nn, "dbias")


@gpu
@pytest.mark.parametrize("layer", ["cheb", "dconv"])
def test_needs_input_grad_prunes(layer):
    """only x needs a gradient: no Z_k is kept and no weight gradient comes back; only the weights need one: no hop runs in the backward"""
    import torch
    import gnnmp
    from gnnmp import backward_poly as B
    if layer == "cheb":
        l, g, x, dY, lam = cheb_layer(3, True, "asymmetric")
        ref, fn, params = R.cheb_ref(3, True, "asymmetric", lam), gnnmp.cheb_conv_ad, lambda: [l.weight, l.bias]      # noqa: E731
    else:
        l, g, x, dY = dconv_layer(3, True)
        ref, fn, params = R.dconv_ref(3, True), gnnmp.d_conv_ad, lambda: [l.weights, l.bias]      # noqa: E731
    hops, hop_fn = [], B.poly_hop
    B.poly_hop = lambda *a, **kw: hops.append(1) or hop_fn(*a, **kw)
    try:
        for p in params():
            p.requires_grad_(False)
            p.grad = None
        xt = dev(x).requires_grad_(True)
        y = fn(l, g, xt)
        fwd = len(hops)
        assert len(y.grad_fn.saved_tensors) == 1      # the weights alone
        y.backward(dev(dY))
        torch.cuda.synchronize()
        assert len(hops) > fwd and all(p.grad is None for p in params())
        close(xt.grad.cpu().numpy(), ref["dx"], "dx")
        for p in params():
            p.requires_grad_(True)
        del hops[:]
        xt = dev(x)
        y = fn(l, g, xt)
        fwd = len(hops)
        y.backward(dev(dY))
        torch.cuda.synchronize()
        assert len(hops) == fwd and xt.grad is None and all(p.grad is not None for p in params())
    finally:
        B.poly_hop = hop_fn


@gpu
def test_the_polynomial_layers_refuse_by_name():
    import torch
    import gnnmp
    l, g, x, dY, _ = cheb_layer(2, True, "none")
    xt = dev(x)
    with pytest.raises(NotImplementedError, match="cheb_conv_ad: a bipartite"):
        gnnmp.cheb_conv_ad(l, g, (xt, xt))
    with pytest.raises(ValueError, match="cheb_conv_ad: the HIP adjoints are Float32"):
        gnnmp.cheb_conv_ad(l, g, xt.double())
    with pytest.raises(ValueError, match="cheb_conv_ad: x must be"):
        gnnmp.cheb_conv_ad(l, g, xt[:, :5].contiguous())
    s, t, n = R.directed_graph()
    directed = gnnmp.GNNGraph(dev(s), dev(t), num_nodes=n, index_base=0)
    with pytest.raises(AssertionError, match="undirected"):      # ChebConv's own check stays
        gnnmp.cheb_conv_ad(l, directed, dev(np.zeros((n, x.shape[1]), f32)))
    ld, gd, xd, _ = dconv_layer(2, False)
    xd = dev(xd)
    with pytest.raises(NotImplementedError, match="d_conv_ad: a bipartite"):
        gnnmp.d_conv_ad(ld, gd, (xd, xd))
    with pytest.raises(ValueError, match="d_conv_ad: the HIP adjoints are Float32"):
        gnnmp.d_conv_ad(ld, gd, xd.double())
    torch.cuda.synchronize()
