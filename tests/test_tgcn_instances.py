"""All sixteen instances of TGCN's one-launch recurrence (csrc/temporal.hip: tgcn_fwd_kernel<NT>, tgcn_bwd_kernel<NT>, NT = ceil(out / 16)
= 1 .. 8) against the float64 restatement of tests/abi_cases.py (tgcn_forward64, tgcn_backward64), through the C ABI with raw pointers
into a poisoned, guarded slab (abi_cases.Slab): every call here also proves that each owed element was written and nothing else was.

  * the table: every NT with a full and a ragged last tile, out % 4 == 0 and != 0, N = 81 (a full block, then a block of one full wave,
    one wave with a single node and two that return early), every h0 / gates / S / dh0 mode at every NT, each call repeated bit for bit;
  * N around the wave and block edges at out = 40, 90, 120 (NT = 3, 6 and the ragged NT = 8 whose last U_h fragments come from L2);
  * the backward judged on its own (y, gates = the float64 forward rounded) and chained behind the forward kernel;
  * a chain of 64 steps, saturated gates, +-Inf in P, a NaN that must stay inside its node, nodes permuted and cut out (bit for bit),
    and the one-launch path against the per-step path at the layer level.

Bound: abi_cases.RTOL = 1e-5 of each reference array's scale, element-wise and norm-wise (abi_cases.compare).  The conditioning guard
(CPU) keeps a float32 numpy restatement of every case within a quarter of that, so the reference's own rounding cannot eat the bound:
hence U ~ N(0, 1) * 0.3 up to out = 64, N(0, 1) * min(0.3, 2 / sqrt(out)) above, and T <= 12 for out > 64."""
import functools
import os
import sys
import zlib
from collections import namedtuple

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_cases as A  # noqa: E402

gpu = pytest.mark.gpu
f32, f64 = np.float32, np.float64
FWD, BWD = "gnnmp_tgcn_recurrence_f32", "gnnmp_tgcn_recurrence_grad_f32"
GUARD = 2.5e-6          # a quarter of A.RTOL: what the float32 restatement may lose against float64, on the array's scale

# ------------------------------------------------------------------------------------------------------------------------------------
# the cases
# ------------------------------------------------------------------------------------------------------------------------------------
TABLE_OUT = {1: (16,), 2: (17, 32), 3: (33, 36, 47, 48), 4: (49, 64), 5: (65, 80), 6: (81, 84, 95, 96), 7: (97, 112), 8: (113, 116, 127, 128)}
OUTS = tuple(o for nt in sorted(TABLE_OUT) for o in TABLE_OUT[nt])
SWEEP_OUT = (40, 90, 120)
SWEEP_N = (1, 15, 16, 17, 63, 64, 65)
CHAIN_OUT = {1: 16, 2: 17, 3: 47, 4: 49, 5: 65, 6: 95, 7: 97, 8: 127}          # forward kernel -> backward kernel, one per NT
H0_MODES = ("null", "vector", "matrix")

# one call: h0 NULL / one vector (h0_stride = 0) / a matrix (h0_stride = out); forward: gates NULL or present; backward: S, dh0 NULL or present
Spec = namedtuple("Spec", "name N T out h0 gates S dh0 pscale")


def nt_of(out):
    return (out + 15) // 16


def out_id(out):
    return f"NT{nt_of(out)}-out{out}-{'full' if out % 16 == 0 else 'ragged'}"


def options(k):
    """the k-th option set of the cycle: consecutive k differ in every option, and any three consecutive k show every value of each"""
    return dict(h0=H0_MODES[k % 3], gates=k % 2 == 0, S=k % 2 == 1, dh0=(k // 2) % 2 == 0)


def table_specs(out):
    """three calls per table entry, the cycle entered at the entry's position in the table"""
    i = OUTS.index(out)
    return [Spec(f"{out_id(out)}-{j}", 81, 3, out, pscale=1.0, **options(i + j)) for j in range(3)]


def sweep_spec(out, N):
    k = SWEEP_OUT.index(out) * len(SWEEP_N) + SWEEP_N.index(N)
    return Spec(f"out{out}-N{N}", N, 3, out, pscale=1.0, **options(k))


def chain_spec(nt):
    return Spec(f"chain-NT{nt}-out{CHAIN_OUT[nt]}", 81, 3, CHAIN_OUT[nt], pscale=1.0, **dict(options(nt), gates=True))


def every(name, N, T, out, pscale=1.0, h0="matrix"):
    return Spec(name, N, T, out, h0, True, True, True, pscale)


LONG = every("long-T64-out40", 33, 64, 40)
SATURATED = [every(f"saturated-out{o}", 70, 3, o, pscale=30.0) for o in SWEEP_OUT]
PERMUTED = [every(f"permuted-out{o}", 130, 3, o) for o in SWEEP_OUT]
POISONED = [every(f"poisoned-out{o}", 81, 4, o) for o in SWEEP_OUT]
ALL_SPECS = ([s for o in OUTS for s in table_specs(o)] + [sweep_spec(o, n) for o in SWEEP_OUT for n in SWEEP_N]
             + [chain_spec(nt) for nt in sorted(CHAIN_OUT)] + [LONG] + SATURATED + PERMUTED + POISONED)
BY_NAME = {s.name: s for s in ALL_SPECS}


def option_coverage():
    """{NT: {(option, value)}} over the table"""
    seen = {}
    for out in OUTS:
        for s in table_specs(out):
            seen.setdefault(nt_of(out), set()).update({("h0", s.h0), ("gates", s.gates), ("S", s.S), ("dh0", s.dh0)})
    return seen


WANTED = {("h0", m) for m in H0_MODES} | {(o, v) for o in ("gates", "S", "dh0") for v in (False, True)}
# at collection, with no GPU: the table reaches every instance, full and ragged, and every instance sees every option
assert sorted(TABLE_OUT) == list(range(1, 9)) and all(nt_of(o) == nt for nt, outs in TABLE_OUT.items() for o in outs)
assert len(OUTS) == 21 and len(BY_NAME) == len(ALL_SPECS)
assert all(any(o % 16 == 0 for o in outs) for outs in TABLE_OUT.values()) and all(any(o % 16 for o in outs) for nt, outs in TABLE_OUT.items() if nt > 1)
assert all(option_coverage()[nt] == WANTED for nt in range(1, 9)), option_coverage()
assert all(nt_of(CHAIN_OUT[nt]) == nt for nt in CHAIN_OUT)


def u_scale(out):
    return 0.3 if out <= 64 else min(0.3, 2.0 / np.sqrt(out))


@functools.lru_cache(maxsize=None)
def data(name):
    """inputs and float64 references of one case, computed once and read-only: P ~ N(0, 1) * pscale, U ~ N(0, 1) * u_scale(out), dy ~ N(0, 1),
    h0 uniform in (-1, 1) (where a state lives); y, gates of the backward = the float64 forward rounded to float32"""
    s = BY_NAME[name]
    N, T, D = s.N, s.T, s.out
    rng = np.random.default_rng(zlib.crc32(repr(("tgcn_instances", N, T, D, s.pscale)).encode()))
    d = dict(P=(rng.standard_normal((N, T, 3 * D)) * s.pscale).astype(f32), Uzr=(rng.standard_normal((2 * D, D)) * u_scale(D)).astype(f32),
             Uh=(rng.standard_normal((D, D)) * u_scale(D)).astype(f32), dy=rng.standard_normal((N, T, D)).astype(f32))
    h0m, h0v = rng.uniform(-1, 1, (N, D)).astype(f32), rng.uniform(-1, 1, D).astype(f32)
    d["h0"] = {"null": None, "vector": h0v, "matrix": h0m}[s.h0]
    d["stride"] = D if s.h0 == "matrix" else 0
    d["y64"], d["gates64"] = A.tgcn_forward64(d["P"], d["Uzr"], d["Uh"], d["h0"], N, T, D)
    d["y"], d["gates"] = d["y64"].astype(f32), d["gates64"].astype(f32)
    d["dP64"], d["S64"], d["dh064"] = A.tgcn_backward64(d["dy"], d["y"], d["gates"], d["Uzr"], d["Uh"], d["h0"], N, T, D)
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


# ---- the same statements in float32 numpy (the conditioning guard's yardstick, never a reference) ---------------------------------
def sigmoid32(x):
    t = np.exp(-np.abs(x))
    return np.where(x >= 0, 1 / (1 + t), t / (1 + t)).astype(f32)


def forward32(P, Uzr, Uh, h0, N, T, D):
    P = P.reshape(N, T, 3 * D)
    h = np.zeros((N, D), f32) if h0 is None else np.broadcast_to(h0, (N, D)).copy()
    y, gates = np.zeros((N, T, D), f32), np.zeros((N, T, 3 * D), f32)
    for t in range(T):
        zr = sigmoid32(P[:, t, :2 * D] + h @ Uzr.T)
        z, r = zr[:, :D], zr[:, D:]
        ht = np.tanh(P[:, t, 2 * D:] + (r * h) @ Uh.T)
        h = (1 - z) * h + z * ht
        y[:, t], gates[:, t] = h, np.concatenate([z, r, ht], 1)
    assert y.dtype == f32 and h.dtype == f32
    return y, gates


def backward32(dy, y, gates, Uzr, Uh, h0, N, T, D):
    Uz, Ur = Uzr[:D], Uzr[D:]
    hstart = np.zeros((N, D), f32) if h0 is None else np.broadcast_to(h0, (N, D))
    dP, S, carry = np.zeros((N, T, 3 * D), f32), np.zeros((N, T, 2 * D), f32), np.zeros((N, D), f32)
    for t in range(T - 1, -1, -1):
        hp = y[:, t - 1] if t else hstart
        z, rr, ht = gates[:, t, :D], gates[:, t, D:2 * D], gates[:, t, 2 * D:]
        dh = dy[:, t] + carry
        ah = dh * z * (1 - ht * ht)
        drh = ah @ Uh
        az = dh * (ht - hp) * z * (1 - z)
        ar = drh * hp * rr * (1 - rr)
        carry = dh * (1 - z) + drh * rr + az @ Uz + ar @ Ur
        dP[:, t], S[:, t] = np.concatenate([az, ar, ah], 1), np.concatenate([hp, rr * hp], 1)
    assert carry.dtype == f32
    return dP, S, carry


def on_scale(got, ref):
    """the worst element of got - ref on the scale of the reference array"""
    return float(np.abs(got.astype(f64) - ref).max() / max(np.abs(ref).max(), 1e-30))


# ------------------------------------------------------------------------------------------------------------------------------------
# CPU
# ------------------------------------------------------------------------------------------------------------------------------------
def test_every_instance_sees_every_option_full_and_ragged():
    cov = option_coverage()
    for nt in range(1, 9):
        assert cov[nt] == WANTED, (nt, WANTED - cov[nt])
        assert any(o % 16 == 0 for o in TABLE_OUT[nt]) and (nt == 1 or any(o % 16 for o in TABLE_OUT[nt]))
    assert {o % 4 == 0 for o in OUTS} == {False, True}
    for nt in (3, 6, 8):                         # the ragged tile ends inside a lane's four columns, and on their edge
        assert {o % 4 == 0 for o in TABLE_OUT[nt] if o % 16} == {False, True}
    # N = 81: block 0 full; block 1 = a full wave, a wave with one node, two waves with none
    waves = (81 + 15) // 16
    assert waves == 6 and (waves + 3) // 4 == 2 and 81 - 80 == 1


def test_the_float64_backward_is_the_pullback_of_the_float64_forward():
    """central differences of tgcn_forward64 in P and h0 against tgcn_backward64 (which the ABI table and every backward test here use)"""
    N, T, D = 3, 3, 5
    rng = np.random.default_rng(3)
    P, Uzr, Uh = rng.standard_normal((N, T, 3 * D)), rng.standard_normal((2 * D, D)) * 0.3, rng.standard_normal((D, D)) * 0.3
    h0, dy = rng.uniform(-1, 1, (N, D)), rng.standard_normal((N, T, D))
    y, gates = A.tgcn_forward64(P, Uzr, Uh, h0, N, T, D)
    dP, S, dh0 = A.tgcn_backward64(dy, y, gates, Uzr, Uh, h0, N, T, D)
    loss = lambda P, h0: float((A.tgcn_forward64(P, Uzr, Uh, h0, N, T, D)[0] * dy).sum())
    eps = 1e-6
    for arr, grad, which in ((P, dP, 0), (h0, dh0, 1)):
        for idx in [tuple(rng.integers(0, n) for n in arr.shape) for _ in range(12)]:
            hi, lo = arr.copy(), arr.copy()
            hi[idx] += eps
            lo[idx] -= eps
            fd = (loss(hi, h0) - loss(lo, h0)) / (2 * eps) if which == 0 else (loss(P, hi) - loss(P, lo)) / (2 * eps)
            assert abs(fd - grad[idx]) <= 1e-7 * max(1.0, np.abs(grad).max()), (which, idx, fd, grad[idx])
    hp = np.concatenate([h0[:, None], y[:, :-1]], 1)
    np.testing.assert_array_equal(S, np.concatenate([hp, gates[:, :, D:2 * D] * hp], 2))


@pytest.mark.parametrize("name", list(BY_NAME))
def test_case_is_well_conditioned(name):
    """a case on which float32 arithmetic itself strays from float64 by more than a quarter of the bound can neither convict nor clear a
    kernel.  (A case that fails here gets a smaller T or U scale, never a wider bound.)"""
    s, d = BY_NAME[name], data(name)
    assert s.out <= 64 or s.T <= 12
    y, gates = forward32(d["P"], d["Uzr"], d["Uh"], d["h0"], s.N, s.T, s.out)
    dP, S, dh0 = backward32(d["dy"], d["y"], d["gates"], d["Uzr"], d["Uh"], d["h0"], s.N, s.T, s.out)
    errs = {"y": on_scale(y, d["y64"]), "gates": on_scale(gates, d["gates64"]), "dP": on_scale(dP, d["dP64"]),
            "S": on_scale(S, d["S64"]), "dh0": on_scale(dh0, d["dh064"])}
    print(name, {k: f"{v:.2e}" for k, v in errs.items()})
    assert max(errs.values()) <= GUARD, errs


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import torch
    assert torch.cuda.is_available()
    from gnnmp import _lib
    return _lib.load()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _launch(lib, export, args, expect, twice=False):
    """one call with every array carved from a fresh poisoned slab, on the current stream.  expect: {output: reference | None}: each owed
    element written, no byte outside the outputs touched, the bound where a reference is given.  twice: the same call again on the
    reloaded slab must give the same bits.  Returns {output: float32 array}"""
    import torch
    case = A.mk(export, "instance", (), args, None)
    slab = A.Slab(case.arrs)
    cargs, _ = A.bind(case, slab, None, torch.cuda.current_stream())
    rc = A.call(lib, case, cargs)
    torch.cuda.synchronize()
    assert rc == A.OK, lib.gnnmp_last_error()
    problems = slab.check({k: A.E(v) for k, v in expect.items()})
    assert not problems, "\n".join(problems)
    after = slab.t.cpu().numpy()
    outs = {k: slab.get(after, k).copy() for k in expect}
    if twice:
        slab.reload()
        assert A.call(lib, case, cargs) == A.OK
        torch.cuda.synchronize()
        again = slab.t.cpu().numpy()
        for k in expect:
            np.testing.assert_array_equal(_bits(slab.get(again, k)), _bits(outs[k]), err_msg=f"'{k}' differs between two runs")
    return outs


def forward(lib, P, Uzr, Uh, h0, stride, N, T, D, want_gates=True, ref=None, twice=False):
    """ref: (y, gates) in float64, or None (memory contract only)"""
    args = [A.Arr("P", "in", P), A.Arr("U_zr", "in", Uzr), A.Arr("U_h", "in", Uh), A.Arr("h0", "in", h0) if h0 is not None else None, stride,
            A.Arr("y", "out", shape=(N, T, D)), A.Arr("gates", "out", shape=(N, T, 3 * D)) if want_gates else None, N, T, D, A.STREAM]
    expect = {"y": None if ref is None else ref[0]}
    if want_gates:
        expect["gates"] = None if ref is None else ref[1]
    return _launch(lib, FWD, args, expect, twice)


def backward(lib, dy, y, gates, Uzr, Uh, h0, stride, N, T, D, want_S=True, want_dh0=True, ref=None, twice=False):
    """ref: (dP, S, dh0) in float64, or None"""
    args = [A.Arr("dy", "in", dy), A.Arr("y", "in", y), A.Arr("gates", "in", gates), A.Arr("U_zr", "in", Uzr), A.Arr("U_h", "in", Uh),
            A.Arr("h0", "in", h0) if h0 is not None else None, stride, A.Arr("dP", "out", shape=(N, T, 3 * D)),
            A.Arr("S", "out", shape=(N, T, 2 * D)) if want_S else None, A.Arr("dh0", "out", shape=(N, D)) if want_dh0 else None, N, T, D, A.STREAM]
    expect = {"dP": None if ref is None else ref[0]}
    if want_S:
        expect["S"] = None if ref is None else ref[1]
    if want_dh0:
        expect["dh0"] = None if ref is None else ref[2]
    return _launch(lib, BWD, args, expect, twice)


def forward_of(lib, s, twice=False):
    d = data(s.name)
    return forward(lib, d["P"], d["Uzr"], d["Uh"], d["h0"], d["stride"], s.N, s.T, s.out, s.gates, (d["y64"], d["gates64"]), twice)


def backward_of(lib, s, twice=False):
    d = data(s.name)
    return backward(lib, d["dy"], d["y"], d["gates"], d["Uzr"], d["Uh"], d["h0"], d["stride"], s.N, s.T, s.out, s.S, s.dh0,
                    (d["dP64"], d["S64"], d["dh064"]), twice)


# ---- the table ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("out", OUTS, ids=out_id)
def test_forward_instance(lib, out):
    for s in table_specs(out):
        forward_of(lib, s, twice=True)


@gpu
@pytest.mark.parametrize("out", OUTS, ids=out_id)
def test_backward_instance(lib, out):
    for s in table_specs(out):
        backward_of(lib, s, twice=True)


@gpu
@pytest.mark.parametrize("N", SWEEP_N)
@pytest.mark.parametrize("out", SWEEP_OUT, ids=out_id)
def test_forward_at_wave_and_block_edges(lib, out, N):
    forward_of(lib, sweep_spec(out, N))


@gpu
@pytest.mark.parametrize("N", SWEEP_N)
@pytest.mark.parametrize("out", SWEEP_OUT, ids=out_id)
def test_backward_at_wave_and_block_edges(lib, out, N):
    backward_of(lib, sweep_spec(out, N))


@gpu
@pytest.mark.parametrize("nt", sorted(CHAIN_OUT), ids=lambda nt: out_id(CHAIN_OUT[nt]))
def test_backward_kernel_behind_the_forward_kernel(lib, nt):
    """end to end: the backward reads what the forward kernel saved, and is compared with the float64 pullback of the float64 forward"""
    s = chain_spec(nt)
    d = data(s.name)
    o = forward_of(lib, s)
    ref = A.tgcn_backward64(d["dy"], d["y64"], d["gates64"], d["Uzr"], d["Uh"], d["h0"], s.N, s.T, s.out)
    backward(lib, d["dy"], o["y"], o["gates"], d["Uzr"], d["Uh"], d["h0"], d["stride"], s.N, s.T, s.out, s.S, s.dh0, ref)


# ---- long chains and extreme inputs ------------------------------------------------------------------------------------------------
@gpu
def test_a_chain_of_64_steps(lib):
    forward_of(lib, LONG)
    backward_of(lib, LONG)


@gpu
@pytest.mark.parametrize("s", SATURATED, ids=lambda s: out_id(s.out))
def test_saturated_gates(lib, s):
    """P ~ N(0, 1) * 30: z, r are 0 or 1 to rounding, z (1 - z) and 1 - h~^2 underflow towards 0"""
    d = data(s.name)
    sat = np.minimum(d["gates64"][..., :2 * s.out], 1 - d["gates64"][..., :2 * s.out]) < 1e-4
    assert sat.mean() > 0.5                       # the case is what it says: more than half of z, r within 1e-4 of 0 or 1
    forward_of(lib, s)
    backward_of(lib, s)


def _poison_site(s):
    """a node in the middle of a full wave, step 1, a column of the ragged last tile"""
    assert s.out % 16 and s.T == 4
    return 24, 1, s.out - 2


@gpu
@pytest.mark.parametrize("s", POISONED, ids=lambda s: out_id(s.out))
def test_infinite_inputs_are_not_poison(lib, s):
    """sigma(+-Inf) is 1 or 0 and tanh(+-Inf) is +-1: finite outputs, at the bound"""
    d = data(s.name)
    n, t, c = _poison_site(s)
    P = d["P"].copy()
    P[n, t, c], P[n + 1, t, s.out + c] = np.inf, -np.inf                      # a_z, a_r
    P[n + 2, t, 2 * s.out + c], P[n + 3, t, c] = np.inf, -np.inf              # a_h, a_z
    P[n + 4, t, 2 * s.out + c - 1], P[n + 4, t, s.out + c] = -np.inf, np.inf  # a_h and a_r of one node
    y64, g64 = A.tgcn_forward64(P, d["Uzr"], d["Uh"], d["h0"], s.N, s.T, s.out)
    assert np.isfinite(y64).all() and np.isfinite(g64).all()
    o = forward(lib, P, d["Uzr"], d["Uh"], d["h0"], d["stride"], s.N, s.T, s.out, ref=(y64, g64))
    assert np.isfinite(o["y"]).all() and np.isfinite(o["gates"]).all()
    assert o["gates"][n, t, c] == 1 and o["gates"][n + 1, t, s.out + c] == 0 and o["gates"][n + 2, t, 2 * s.out + c] == 1
    y, g = y64.astype(f32), g64.astype(f32)
    backward(lib, d["dy"], y, g, d["Uzr"], d["Uh"], d["h0"], d["stride"], s.N, s.T, s.out,
             ref=A.tgcn_backward64(d["dy"], y, g, d["Uzr"], d["Uh"], d["h0"], s.N, s.T, s.out))


def _contained(name, got, clean, ref, n, t_nan, forward_in_time):
    """node n: NaN exactly where the float64 reference is (A.compare, run by the call, has already asserted that and the bound on the
    rest); it IS NaN from the poisoned step on; every other node carries the bits of the clean run"""
    others = np.arange(got.shape[0]) != n
    np.testing.assert_array_equal(_bits(got[others]), _bits(clean[others]), err_msg=f"'{name}': a NaN in node {n} changed another node")
    np.testing.assert_array_equal(np.isnan(got[n]), np.isnan(ref[n]), err_msg=f"'{name}': NaN pattern of node {n}")
    if got.ndim == 3:
        before = slice(0, t_nan) if forward_in_time else slice(t_nan + 1, None)
        np.testing.assert_array_equal(_bits(got[n, before]), _bits(clean[n, before]), err_msg=f"'{name}': node {n} changed before the NaN arrived")


@gpu
@pytest.mark.parametrize("s", POISONED, ids=lambda s: out_id(s.out))
def test_a_nan_stays_inside_its_node_forward(lib, s):
    d = data(s.name)
    n, t, c = _poison_site(s)
    P = d["P"].copy()
    P[n, t, c] = np.nan
    y64, g64 = A.tgcn_forward64(P, d["Uzr"], d["Uh"], d["h0"], s.N, s.T, s.out)
    assert np.isnan(y64[n, t, c]) and np.isnan(y64[n, t]).sum() == 1 and np.isnan(y64[n, t + 1:]).all() and np.isnan(g64[n, t + 1:]).all()
    assert not np.isnan(np.delete(y64, n, 0)).any() and not np.isnan(y64[n, :t]).any()
    clean = forward_of(lib, s)
    o = forward(lib, P, d["Uzr"], d["Uh"], d["h0"], d["stride"], s.N, s.T, s.out, ref=(y64, g64))
    _contained("y", o["y"], clean["y"], y64, n, t, True)
    _contained("gates", o["gates"], clean["gates"], g64, n, t, True)


@gpu
@pytest.mark.parametrize("s", POISONED, ids=lambda s: out_id(s.out))
def test_a_nan_stays_inside_its_node_backward(lib, s):
    d = data(s.name)
    n, t, c = _poison_site(s)
    dy = d["dy"].copy()
    dy[n, t, c] = np.nan
    ref = A.tgcn_backward64(dy, d["y"], d["gates"], d["Uzr"], d["Uh"], d["h0"], s.N, s.T, s.out)
    assert np.isnan(ref[0][n, :t]).all() and np.isnan(ref[2][n]).all() and not np.isnan(ref[0][n, t + 1:]).any() and not np.isnan(ref[1]).any()
    assert not np.isnan(np.delete(ref[0], n, 0)).any() and not np.isnan(np.delete(ref[2], n, 0)).any()
    clean = backward_of(lib, s)
    o = backward(lib, dy, d["y"], d["gates"], d["Uzr"], d["Uh"], d["h0"], d["stride"], s.N, s.T, s.out, ref=ref)
    for k, r in zip(("dP", "S", "dh0"), ref):
        _contained(k, o[k], clean[k], r, n, t, False)


# ---- a node's arithmetic depends on neither its position nor its wave-mates ---------------------------------------------------------
def _rows(d, keys, idx):
    return {k: np.ascontiguousarray(d[k][idx]) for k in keys}


@gpu
@pytest.mark.parametrize("s", PERMUTED, ids=lambda s: out_id(s.out))
def test_nodes_are_independent_bit_for_bit(lib, s):
    """130 nodes; the same nodes in a fixed random order; nodes 64 .. 129 alone.  Every output row must come back with the same bits: lane
    n of the MFMA's B operand and C / D tile is node n and nothing else, whichever wave, tile position and neighbours it has"""
    d = data(s.name)
    N, T, D = s.N, s.T, s.out
    perm = np.random.default_rng(130).permutation(N)
    tail = np.arange(64, N)
    assert (perm != np.arange(N)).sum() > 100 and (perm // 16 != np.arange(N) // 16).sum() > 100
    U = (d["Uzr"], d["Uh"])

    def fwd(idx):
        a = _rows(d, ("P", "h0"), idx)
        return forward(lib, a["P"], *U, a["h0"], D, len(idx), T, D)

    def bwd(idx):
        a = _rows(d, ("dy", "y", "gates", "h0"), idx)
        return backward(lib, a["dy"], a["y"], a["gates"], *U, a["h0"], D, len(idx), T, D)

    for run, ref in ((fwd, (d["y64"], d["gates64"])), (bwd, (d["dP64"], d["S64"], d["dh064"]))):
        base, shuffled, cut = run(np.arange(N)), run(perm), run(tail)
        for k, r in zip(base, ref):
            assert A.compare(base[k], r, A.E()) is None
            back = np.empty_like(shuffled[k])
            back[perm] = shuffled[k]
            np.testing.assert_array_equal(_bits(back), _bits(base[k]), err_msg=f"'{k}' depends on where a node sits")
            np.testing.assert_array_equal(_bits(cut[k]), _bits(base[k][tail]), err_msg=f"'{k}' of nodes 64.. depends on nodes 0..63")


# ---- padding stays inert ------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("out", SWEEP_OUT, ids=out_id)
def test_ragged_tiles_write_what_they_owe_and_nothing_else(lib, out):
    """(every call of this file runs in the slab; here without a reference, so that the memory contract is reported on its own: y, gates, dP,
    S and dh0 start as NaN poison inside 4 KiB guard bands, the last tile's padded columns lie over the next row / the band)"""
    s = sweep_spec(out, 65)
    d = data(s.name)
    assert out % 16 and A.GUARD_MIN >= 4096
    o = forward(lib, d["P"], d["Uzr"], d["Uh"], d["h0"], d["stride"], s.N, s.T, out)
    assert all(np.isfinite(v).all() for v in o.values())
    o = backward(lib, d["dy"], d["y"], d["gates"], d["Uzr"], d["Uh"], d["h0"], d["stride"], s.N, s.T, out)
    assert all(np.isfinite(v).all() for v in o.values())


# ---- the layer: one launch against one launch per step ------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("out", SWEEP_OUT, ids=out_id)
def test_one_launch_and_per_step_paths_agree(out):
    import torch
    import gnnmp
    from gnnmp import _lib
    from test_tgcn import close, road_graph
    n, T = 70, 4
    s1, t1 = road_graph(n, seed=9)
    g = gnnmp.GNNGraph(torch.from_numpy(s1).cuda(), torch.from_numpy(t1).cuda(), num_nodes=n)
    layer = gnnmp.TGCN((2, out), seed=4)
    gen = torch.Generator().manual_seed(out)
    x, st = torch.randn((n, T, 2), generator=gen).cuda(), torch.randn((n, out), generator=gen).cuda()
    dy = torch.randn((n, T, out), generator=gen).cuda()

    def run():
        xd, sd = x.clone().requires_grad_(), st.clone().requires_grad_()
        for p in layer.cell.parameters():
            p.requires_grad_()
        y = gnnmp.tgcn_ad(layer, g, xd, sd)
        return [y.detach()] + list(torch.autograd.grad(y, [xd, sd] + layer.cell.parameters(), dy))

    a = run()
    with _lib.tuned(_lib.Knob.TGCN, -1):
        b = run()
    assert len(a) == 21
    for k, (u, v) in enumerate(zip(a, b)):
        close(u, v, f"one launch vs per step, output {k}", rtol=A.RTOL)
