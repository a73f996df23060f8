"""set2set_ad and global_attention_pool_ad: the attention readouts trained on the fused segment kernels (csrc/readout.hip; include/gnnmp.h
states the arithmetic), and the pullback of the LSTM cell's pointwise part.

Without a GPU: the three exports exist in header, SYMBOLS and library and take const host records whose ctypes mirrors have the header's
layout; every refusal of the header comes before any HIP call; G = 0 and N = 0 return OK; the float64 reference (tests/readout_ref.py)
agrees with central finite differences (Set2Set at 1 and 3 iterations, GlobalAttentionPool with a gate of 1 and of D' channels, with and
without ffeat), with oracle.more_layers.set2set_pool and with the oracle composition of tests/test_attention_pool.py; the operands of
every GPU case keep the float32 restatement of the header's formulas within 2e-6 of float64 and relu's pre-activations 1e-3 from 0; the
Python-level refusals.

On the GPU: every export within 1e-5 of float64, norm-wise and element-wise, at every lane-group width, vector tail and tile count, on
segments of 1, 2, 5, 63, 64, 65, 3 and 700 rows with an empty segment in the middle and one at the end; pruned outputs leave the others'
bits alone; base aliasing dx; equal bits of two calls; every output element written and nothing else at any pointer alignment; each
export recorded into a HIP graph without an eager call first; the two layers against the reference, the oracle and the existing
forwards; dx at 1e-5; weight and bias gradients by readout_ref.weight_bar; pruning; one MPNN step."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_cases as A  # noqa: E402
import readout_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POOL, GRAD, LSTM = "gnnmp_segment_attn_pool_f32", "gnnmp_segment_attn_pool_grad_f32", "gnnmp_lstm_pointwise_grad_f32"
gpu = pytest.mark.gpu
f32, f64 = np.float32, np.float64
RECORDS = {POOL: ("gnnmp_segment_attn_t", "SegmentAttnJob", ("x", "seg_ptr", "q", "gate", "r", "stats")),
           GRAD: ("gnnmp_segment_attn_grad_t", "SegmentAttnGradJob",
                  ("dr", "x", "seg_ptr", "q", "gate", "r", "stats", "base", "dq", "dx", "dgate")),
           LSTM: ("gnnmp_lstm_grad_t", "LstmGradJob", ("gx", "gh", "b", "c", "dh", "dcn", "da", "dc"))}
PARAMS = {POOL: ["job", "N", "G", "D", "Dg", "stream"], GRAD: ["job", "N", "G", "D", "Dg", "stream"], LSTM: ["job", "N", "D", "stream"]}
MODES = ("query", "one", "all")      # Dg = 0, 1, D


def dg_of(mode, D):
    return {"query": 0, "one": 1, "all": D}[mode]


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
    for name in (POOL, GRAD, LSTM):
        assert f"int {name}(" in header and header.index(f"int {name}(") < internal, name
        assert name in _lib.SYMBOLS and name in exported, name
        assert "} " + RECORDS[name][0] + ";" in header
    assert "GNNlib/src/layers/pool.jl:7-12" in header[:internal] and "pool.jl:29-43" in header[:internal]
    assert "tests/test_readout_ad.py" in header[:header.index("#ifndef GNNMP_H")]           # the Conventions paragraph: what is tested
    assert f"#define GNNMP_READOUT_MAX_D {_lib.READOUT_MAX_D}\n" in header and _lib.READOUT_MAX_D >= 1024
    assert callable(gnnmp.set2set_ad) and callable(gnnmp.global_attention_pool_ad)


@pytest.mark.parametrize("export", [POOL, GRAD, LSTM])
def test_the_exports_take_const_host_records(export):
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
        assert "*" in decl, decl      # these records hold pointers only
        for nme in [n.strip().lstrip("*") for n in re.sub(r"^(const\s+)?(float|int64_t)\s+", "", decl).split(",")]:
            fields.append(nme)
            offsets.append(off)
            off += 8
    rec = getattr(_lib, cls)
    assert tuple(fields) == want == tuple(f for f, _ in rec._fields_)
    assert [getattr(rec, f).offset for f in want] == offsets
    assert ctypes.sizeof(rec) == off


P_ = lambda v: ctypes.c_void_p(0x1000 * v) if v else None      # never dereferenced: the call must refuse first  # noqa: E731


def _pool(lib, job=True, x=1, seg_ptr=2, q=3, gate=None, r=5, stats=6, N=7, G=2, D=4, Dg=0):
    from gnnmp import _lib
    j = _lib.SegmentAttnJob(P_(x), P_(seg_ptr), P_(q), P_(gate), P_(r), P_(stats))
    return lib.gnnmp_segment_attn_pool_f32(ctypes.byref(j) if job else None, N, G, D, Dg, None)


def _grad(lib, job=True, dr=1, x=2, seg_ptr=3, q=4, gate=None, r=6, stats=7, base=None, dq=9, dx=10, dgate=None, N=7, G=2, D=4, Dg=0):
    from gnnmp import _lib
    j = _lib.SegmentAttnGradJob(P_(dr), P_(x), P_(seg_ptr), P_(q), P_(gate), P_(r), P_(stats), P_(base), P_(dq), P_(dx), P_(dgate))
    return lib.gnnmp_segment_attn_pool_grad_f32(ctypes.byref(j) if job else None, N, G, D, Dg, None)


def _lstm(lib, job=True, gx=1, gh=2, b=3, c=4, dh=5, dcn=6, da=7, dc=8, N=3, D=4):
    from gnnmp import _lib
    j = _lib.LstmGradJob(P_(gx), P_(gh), P_(b), P_(c), P_(dh), P_(dcn), P_(da), P_(dc))
    return lib.gnnmp_lstm_pointwise_grad_f32(ctypes.byref(j) if job else None, N, D, None)


GATE = dict(q=None, gate=4)


def test_argument_validation_needs_no_gpu():
    """every refusal of the header comes before the first HIP call — on a machine without a device, on pointers that are not memory — and
    names its export"""
    from gnnmp import _lib
    lib = _lib.load()
    EINVAL, err = _lib.EINVAL, lib.gnnmp_last_error
    big = _lib.READOUT_MAX_D
    for fn, who, req in ((_pool, b"segment_attn_pool:", ("x", "seg_ptr", "r", "stats")),
                         (_grad, b"segment_attn_pool_grad:", ("dr", "x", "seg_ptr", "r", "stats"))):
        assert fn(lib, job=False) == EINVAL and who + b" null job" in err()
        for name in req:
            assert fn(lib, **{name: None}) == EINVAL and who + f" null {name}".encode() in err(), name
        assert fn(lib, gate=4) == EINVAL and who in err() and b"exactly one of q and gate" in err()
        assert fn(lib, q=None) == EINVAL and who in err() and b"exactly one of q and gate" in err()
        for Dg in (-1, 2, 3, 5, 2 ** 40):
            assert fn(lib, Dg=Dg) == EINVAL and who in err() and b"bad Dg" in err(), Dg
        assert fn(lib, Dg=1) == EINVAL and who in err() and b"does not go with q" in err()
        assert fn(lib, Dg=4) == EINVAL and b"does not go with q" in err()
        assert fn(lib, Dg=0, **GATE) == EINVAL and who in err() and b"does not go with gate" in err()
        for D in (0, -1, big + 1, 2 ** 40):
            assert fn(lib, D=D) == EINVAL and who in err() and b"bad D" in err(), D
        assert fn(lib, N=-1) == EINVAL and who in err() and b"negative" in err()
        assert fn(lib, G=-1) == EINVAL and who in err() and b"negative" in err()
    assert _grad(lib, dq=None, dx=None) == EINVAL and b"segment_attn_pool_grad: dq and dx are both null" in err()
    assert _grad(lib, dgate=11) == EINVAL and b"dgate in query mode" in err()
    assert _grad(lib, Dg=1, dq=None, dx=None, **GATE) == EINVAL and b"dgate and dx are both null" in err()
    assert _grad(lib, Dg=1, dgate=11, **GATE) == EINVAL and b"dq in gate mode" in err()
    assert _grad(lib, base=8, dx=None) == EINVAL and b"base without dx" in err()
    who = b"lstm_pointwise_grad:"
    assert _lstm(lib, job=False) == EINVAL and who + b" null job" in err()
    for name in ("gx", "gh", "c", "dh", "da", "dc"):
        assert _lstm(lib, **{name: None}) == EINVAL and who in err() and b"null" in err(), name
    for D in (0, -1, (1 << 20) + 1):
        assert _lstm(lib, D=D) == EINVAL and who in err() and b"bad D" in err(), D
    assert _lstm(lib, N=-1) == EINVAL and who in err() and b"negative N" in err()


def test_empty_sizes_return_ok_without_a_device():
    """G = 0 and N = 0 launch nothing, in every mode, at the widest D, with and without the optional pointers"""
    from gnnmp import _lib
    lib = _lib.load()
    big = _lib.READOUT_MAX_D
    for kw in (dict(G=0), dict(N=0), dict(N=0, G=0), dict(N=0, x=None)):
        assert _pool(lib, **kw) == _lib.OK
        assert _pool(lib, D=big, **kw) == _lib.OK
        assert _pool(lib, Dg=1, **GATE, **kw) == _lib.OK
        assert _pool(lib, Dg=4, **GATE, **kw) == _lib.OK
        assert _grad(lib, **kw) == _lib.OK
        assert _grad(lib, dq=None, base=8, **kw) == _lib.OK
        assert _grad(lib, dx=None, D=big, **kw) == _lib.OK
        assert _grad(lib, Dg=1, dq=None, dgate=11, **GATE, **kw) == _lib.OK
        assert _grad(lib, Dg=4, dq=None, dx=None, dgate=11, **GATE, **kw) == _lib.OK
    assert _lstm(lib, N=0) == _lib.OK
    assert _lstm(lib, N=0, b=None, dcn=None, D=1 << 20) == _lib.OK


# ------------------------------------------------------------------------------------------------------------------------------------
# CPU: the references
# ------------------------------------------------------------------------------------------------------------------------------------
FD_SEGS = (2, 3, 1, 4)


def fd_check(arrays, loss, h=1e-6):
    for arr, g, what in arrays:
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


@pytest.mark.parametrize("iters", [1, 3])
def test_set2set_reference_agrees_with_finite_differences(iters):
    """central differences of the float64 layer, h = 1e-6, loss = Σ out ⊙ R: dx, dWi, dWh, db"""
    x, ptr, Wi, Wh, b, dout = [np.array(a, f64) if a.dtype == f32 else a for a in R.set2set_case(3, 5, FD_SEGS)]
    ref = R.set2set_grad(x, ptr, Wi, Wh, b, iters, dout)
    fd_check([(x, ref["dx"], "dx"), (Wi, ref["dWi"], "dWi"), (Wh, ref["dWh"], "dWh"), (b, ref["db"], "db")],
             lambda: float((R.set2set(x, ptr, Wi, Wh, b, iters)[0] * dout).sum()))


@pytest.mark.parametrize("Dg,with_ffeat", R.GAP_VARIANTS)
def test_attention_pool_reference_agrees_with_finite_differences(Dg, with_ffeat):
    """dx and every weight and bias of fgate and ffeat; relu's pre-activations are 1e-3 = 1000 h from their kinks (R.gap_case)"""
    x, ptr, fgate, ffeat, dr = R.gap_case(4, Dg, with_ffeat, FD_SEGS)
    x, dr, fgate, ffeat = np.array(x, f64), np.array(dr, f64), R.chain64(fgate), R.chain64(ffeat)
    ref = R.gap_grad(x, ptr, fgate, ffeat, dr)
    arrays = [(x, ref["dx"], "dx")]
    for name, chain in (("fgate", fgate), ("ffeat", ffeat or [])):
        for k, (W, b, _) in enumerate(chain):
            arrays += [(W, ref[name][k][0], f"{name}[{k}].W"), (b, ref[name][k][1], f"{name}[{k}].b")]
    fd_check(arrays, lambda: float((R.gap(x, ptr, fgate, ffeat)[0] * dr).sum()))


def test_export_references_agree_with_finite_differences():
    """the two segment formulas and the LSTM pullback, each against central differences of its own forward, float64"""
    for Dg in (0, 1, 3):
        x, ptr, q, gate, dr, base = R.cast(f64, *R.pool_case(3, Dg, 1, (2, 0, 3, 1)))
        ptr = ptr.astype(np.int64)
        r, stats = R.pool(x, ptr, q, gate)
        dq, dx, dgate = R.pool_grad(dr, x, ptr, r, stats, q, gate)
        arrays = [(x, dx, "dx")] + ([(q, dq, "dq")] if Dg == 0 else [(gate, dgate, "dgate")])
        fd_check(arrays, lambda: float((R.pool(x, ptr, q, gate)[0] * dr).sum()))
        assert not r[1].any() and not stats[1].any() and (Dg or not dq[1].any())      # the empty segment
    gx, gh, b, c, dh, dcn = R.cast(f64, *R.lstm_case(4, 3))
    da, dc = R.lstm_grad(gx, gh, b, c, dh, dcn)

    def loss():
        h, cn = R.lstm(gx, gh, b, c)
        return float((h * dh).sum() + (cn * dcn).sum())
    fd_check([(gx, da, "da (gx)"), (gh, da, "da (gh)"), (b, da.sum(axis=0), "db"), (c, dc, "dc")], loss)


@pytest.mark.parametrize("iters", [1, 3])
@pytest.mark.parametrize("n", [3, 64])
def test_set2set_reference_agrees_with_the_oracle(n, iters):
    from oracle import more_layers as ML
    x, ptr, Wi, Wh, b, _ = R.set2set_case(n)
    want = R.set2set_ref(n, iters)["y"]
    got = ML.set2set_pool(R.indicator(R.SEGS), len(R.SEGS), x, Wi, Wh, b, iters)
    assert R.rel(got, want) <= 1e-5 and R.worst(got, want) <= 1e-5


def oracle_gap(orc, x, fgate, ffeat):
    """the composition of tests/test_attention_pool.py: the pinned helpers of the oracle"""
    from oracle import graphwise as GW
    gi, G = R.indicator(R.SEGS), len(R.SEGS)

    def chain(h, layers):
        for W, b, act in layers:
            h = orc.matmul(W, h) + b[None, :]
            h = orc._act("relu", h) if act == "relu" else h
        return h.astype(f32)
    feats = chain(x, ffeat) if ffeat else x
    alpha = GW.softmax_nodes(gi, chain(x, fgate), G)
    return orc.scatter("+", (alpha * feats).astype(f32), gi, G)


@pytest.mark.parametrize("Dg,with_ffeat", R.GAP_VARIANTS)
def test_attention_pool_reference_agrees_with_the_oracle(oracle, Dg, with_ffeat):
    x, ptr, fgate, ffeat, _ = R.gap_case(10, Dg, with_ffeat)
    want = R.gap_ref(10, Dg, with_ffeat)["y"]
    got = oracle_gap(oracle, x, fgate, ffeat)
    assert R.rel(got, want) <= 1e-5 and R.worst(got, want) <= 1e-5


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("D", R.WIDTHS)
def test_the_export_cases_are_well_conditioned(D, mode):
    """THE CONDITION ON THE INPUTS, not a measurement of the kernels: r, stats, dq, dx, dgate by the header's formulas in float32 are
    within 2e-6, norm-wise, of float64"""
    dist = R.pool_condition(D, dg_of(mode, D))
    print(f"D = {D}, {mode}: the float32 restatement is {dist:.2e} from float64")
    assert dist <= R.COND


LAYER_N = (3, 64)
LAYER_ITERS = (1, 3)
GAP_D = 10


def test_the_layer_cases_are_well_conditioned():
    """the float32 restatement of both layers stays within 2e-6 of float64 in y and dx; relu's pre-activations 1e-3 from 0; prints how much
    of the fp32 summation bound γ_n Σ|terms| the restatement's weight gradients use (what weight_bar decides by)"""
    for n in LAYER_N:
        for iters in LAYER_ITERS:
            ref, rest = R.set2set_ref(n, iters), R.set2set_ref(n, iters, dtype="float32")
            dist = max(R.rel(rest[k], ref[k]) for k in ("y", "dx"))
            used = {k: R.bound_used(rest[k], ref[k], ref[m], ref["n"]) for k, m in (("dWi", "mWi"), ("dWh", "mWh"), ("db", "mb"))}
            print(f"Set2Set n_in = {n}, {iters} iteration(s): restatement {dist:.2e} from float64; bound used {used}")
            assert dist <= R.COND
    for Dg, with_ffeat in R.GAP_VARIANTS:
        ref, rest = R.gap_ref(GAP_D, Dg, with_ffeat), R.gap_ref(GAP_D, Dg, with_ffeat, dtype="float32")
        dist = max(R.rel(rest[k], ref[k]) for k in ("y", "dx"))
        kink = min(float(np.abs(p).min()) for p in ref["pres"])
        print(f"GlobalAttentionPool gate {Dg}, ffeat {with_ffeat}: restatement {dist:.2e} from float64, kink {kink:.2e}")
        assert dist <= R.COND and kink >= R.KINK


class _NotDense:
    sigma = None


def test_python_level_refusals():
    """ValueError, by name, before any launch (no graph is touched: g = None)"""
    import torch
    import gnnmp
    from gnnmp.layers_khop import GlobalAttentionPool
    mk = lambda ch, sigma=None: gnnmp.Dense(ch, sigma, device="cpu", seed=1)      # noqa: E731
    x = torch.zeros((5, 4), dtype=torch.float32)
    ok = mk((4, 1))
    with pytest.raises(ValueError, match="global_attention_pool_ad: layer 1 of fgate is a _NotDense"):
        gnnmp.global_attention_pool_ad(GlobalAttentionPool([mk((4, 4)), _NotDense()]), None, x)
    with pytest.raises(ValueError, match="global_attention_pool_ad: layer 0 of ffeat is a _NotDense"):
        gnnmp.global_attention_pool_ad(GlobalAttentionPool(ok, _NotDense()), None, x)
    for sigma in ("tanh", "swish", torch.sigmoid):
        with pytest.raises(ValueError, match="global_attention_pool_ad: σ = .* in fgate"):
            gnnmp.global_attention_pool_ad(GlobalAttentionPool(mk((4, 1), sigma)), None, x)
        with pytest.raises(ValueError, match="global_attention_pool_ad: σ = .* in ffeat"):
            gnnmp.global_attention_pool_ad(GlobalAttentionPool(ok, [mk((4, 4), "relu"), mk((4, 3), sigma)]), None, x)
    with pytest.raises(ValueError, match="global_attention_pool_ad: Float32 only"):
        gnnmp.global_attention_pool_ad(GlobalAttentionPool(ok), None, x.double())
    with pytest.raises(ValueError, match="the gate has 2 channels"):
        gnnmp.global_attention_pool_ad(GlobalAttentionPool(mk((4, 2))), None, x)
    with pytest.raises(ValueError, match="the gate has 4 channels.*\\(3\\)"):
        gnnmp.global_attention_pool_ad(GlobalAttentionPool(mk((4, 4)), mk((4, 3))), None, x)
    with pytest.raises(ValueError, match="global_attention_pool_ad: fgate is empty"):
        gnnmp.global_attention_pool_ad(GlobalAttentionPool([]), None, x)
    s2s = gnnmp.Set2Set(4, 2, device="cpu", seed=1)
    with pytest.raises(ValueError, match="set2set_ad: Float32 only"):
        gnnmp.set2set_ad(s2s, None, x.double())
    with pytest.raises(ValueError, match="set2set_ad: x has 3 features, the LSTM cell was built for 4"):
        gnnmp.set2set_ad(s2s, None, x[:, :3])
    with pytest.raises(ValueError, match="set2set_ad: x must be"):
        gnnmp.set2set_ad(s2s, None, x[:, 0])


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU helpers
# ------------------------------------------------------------------------------------------------------------------------------------
def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def close(got, ref, what, tol=1e-5):
    """the project's parity bar, norm-wise AND element-wise against the array scale (tests/test_megnet_conv_ad.py: close)"""
    got, ref = np.asarray(got, f64), np.asarray(ref, f64)
    assert got.shape == ref.shape, what
    assert np.all(np.isfinite(got)), f"{what}: non-finite"
    err, scale = np.linalg.norm(got - ref), np.linalg.norm(ref)
    worst = np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300) if ref.size else 0.0
    print(f"{what}: |got - ref| = {err:.3e}, |ref| = {scale:.3e}, ratio {err / max(scale, 1e-300):.2e}, element-wise {worst:.2e}")
    assert err <= tol * scale, f"{what}: {err:.3e} > {tol:g} * {scale:.3e}"
    assert worst <= tol, f"{what}: element-wise {worst:.2e} of the array scale"


def judge(got, rest, ref, mag, n, what):
    """a weight or bias gradient against float64 by readout_ref.weight_bar: inside the fp32 summation bound γ_n Σ|terms|, or — where the
    float32 restatement on the CPU is not inside it itself — within 4 × the restatement's own distance"""
    kind, bar = R.weight_bar(rest, ref, mag, n)
    got = np.asarray(got, f64)
    assert got.shape == np.shape(ref) and np.all(np.isfinite(got)), what
    if kind == "sum":
        used = R.bound_used(got, ref, mag, n)
        print(f"{what}: uses {used:.3f} of the summation bound (n = {n})")
        assert np.all(np.abs(got - ref) <= bar), f"{what}: {used:.2f} of the summation bound"
    else:
        print(f"{what}: the restatement leaves the summation bound; bar {bar:.2e} = 4 x its distance from float64")
        close(got, ref, what, tol=bar)


def ptr(v):
    return None if v is None else ctypes.c_void_p(v.data_ptr())


def call_pool(lib, x, sp, q, gate, r, stats, N, G, D, Dg, stream=None):
    from gnnmp import _lib
    job = _lib.SegmentAttnJob(x, sp, q, gate, r, stats)
    return lib.gnnmp_segment_attn_pool_f32(ctypes.byref(job), N, G, D, Dg, stream)


def call_grad(lib, dr, x, sp, q, gate, r, stats, base, dq, dx, dgate, N, G, D, Dg, stream=None):
    from gnnmp import _lib
    job = _lib.SegmentAttnGradJob(dr, x, sp, q, gate, r, stats, base, dq, dx, dgate)
    return lib.gnnmp_segment_attn_pool_grad_f32(ctypes.byref(job), N, G, D, Dg, stream)


def call_lstm(lib, gx, gh, b, c, dh, dcn, da, dc, N, D, stream=None):
    from gnnmp import _lib
    job = _lib.LstmGradJob(gx, gh, b, c, dh, dcn, da, dc)
    return lib.gnnmp_lstm_pointwise_grad_f32(ctypes.byref(job), N, D, stream)


@pytest.fixture(scope="module")
def lib():
    import torch
    assert torch.cuda.is_available()
    from gnnmp import _lib
    return _lib.load()


def nan(*shape):
    import torch
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def run_pool(lib, D, Dg):
    import torch
    x, sp, q, gate, _, _ = R.pool_case(D, Dg)
    N, G = x.shape[0], len(sp) - 1
    xd, spd, qd, gd = dev(x), dev(sp), None if q is None else dev(q), None if gate is None else dev(gate)
    r, stats = nan(G, D), nan(G, max(Dg, 1), 2)
    rc = call_pool(lib, ptr(xd), ptr(spd), ptr(qd), ptr(gd), ptr(r), ptr(stats), N, G, D, Dg)
    assert rc == A.OK, lib.gnnmp_last_error()
    torch.cuda.synchronize()
    return r.cpu().numpy(), stats.cpu().numpy()


def run_grad(lib, D, Dg, r, stats, base=None, want=("dq", "dx", "dgate")):
    """(dq, dx, dgate), None where the mode has none or `want` leaves it out; base: None | 'separate' | 'alias'"""
    import torch
    x, sp, q, gate, dr, b = R.pool_case(D, Dg)
    N, G = x.shape[0], len(sp) - 1
    xd, spd, qd, gd = dev(x), dev(sp), None if q is None else dev(q), None if gate is None else dev(gate)
    dq = nan(G, D) if Dg == 0 and "dq" in want else None
    dgate = nan(N, Dg) if Dg and "dgate" in want else None
    dx = (dev(b) if base == "alias" else nan(N, D)) if "dx" in want else None
    bd = None if base is None else dx if base == "alias" else dev(b)
    drd, rd, sd = dev(dr), dev(r), dev(stats)
    rc = call_grad(lib, ptr(drd), ptr(xd), ptr(spd), ptr(qd), ptr(gd), ptr(rd), ptr(sd), ptr(bd), ptr(dq), ptr(dx), ptr(dgate), N, G, D, Dg)
    assert rc == A.OK, lib.gnnmp_last_error()
    torch.cuda.synchronize()
    return tuple(None if v is None else v.cpu().numpy() for v in (dq, dx, dgate))


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU 1: the exports against float64
# ------------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("D", R.WIDTHS)
def test_segment_exports_against_float64(lib, D, mode):
    """D = 1, 3, 5, 33: 4-byte lanes, groups of 1, 4, 8, 64; 2, 130: 8-byte lanes (130: 65 lanes, a second tile with one active lane); 4, 8,
    64, 100, 260: 16-byte lanes, groups of 1, 2, 16, 32 (25 active) and 64 (260: a second tile).  r, stats, dq, dx, dgate within 1e-5 of
    float64; the empty segments (4 and 9) give r = 0, stats = 0 and dq = 0; pruned outputs leave the others' bits alone; base == dx gives
    the bits of a separate base; two calls give equal bits"""
    Dg = dg_of(mode, D)
    ref = R.pool_ref(D, Dg)
    r, stats = run_pool(lib, D, Dg)
    close(r, ref["r"], "r")
    close(stats, ref["stats"], "stats")
    empty = [g for g, n in enumerate(R.SEGS_ABI) if n == 0]
    assert len(empty) == 2 and not r[empty].any() and not stats[empty].any()
    r2, stats2 = run_pool(lib, D, Dg)
    assert np.array_equal(bits(r), bits(r2)) and np.array_equal(bits(stats), bits(stats2))
    dq, dx, dgate = run_grad(lib, D, Dg, r, stats)
    close(dx, ref["dx"], "dx")
    if mode == "query":
        close(dq, ref["dq"], "dq")
        assert dgate is None and not dq[empty].any()
    else:
        close(dgate, ref["dgate"], "dgate")
        assert dq is None
    other = "dq" if mode == "query" else "dgate"
    again = run_grad(lib, D, Dg, r, stats)
    only_dx = run_grad(lib, D, Dg, r, stats, want=("dx",))
    only_other = run_grad(lib, D, Dg, r, stats, want=(other,))
    for k, full in enumerate((dq, dx, dgate)):
        if full is not None:
            assert np.array_equal(bits(again[k]), bits(full))
    assert np.array_equal(bits(only_dx[1]), bits(dx)) and only_dx[0] is None and only_dx[2] is None
    assert only_other[1] is None and np.array_equal(bits(only_other[0 if mode == "query" else 2]), bits(dq if mode == "query" else dgate))
    sep = run_grad(lib, D, Dg, r, stats, base="separate")
    alias = run_grad(lib, D, Dg, r, stats, base="alias")
    close(sep[1], ref["dx_base"], "dx with base")
    for a, b_ in zip(sep, alias):
        assert (a is None and b_ is None) or np.array_equal(bits(a), bits(b_))
    assert np.array_equal(bits(sep[0 if mode == "query" else 2]), bits(dq if mode == "query" else dgate))


LSTM_SHAPES = [(1, 1), (8, 3), (5, 64), (300, 33)]


def lstm_ref(N, D, seed=0, with_opt=True):
    gx, gh, b, c, dh, dcn = R.cast(f64, *R.lstm_case(N, D, seed))
    return R.lstm_grad(gx, gh, b if with_opt else None, c, dh, dcn if with_opt else None)


@gpu
@pytest.mark.parametrize("N,D", LSTM_SHAPES)
def test_lstm_pointwise_grad_against_float64(lib, N, D):
    """da, dc within 1e-5 of float64 with and without b and dcn; the gates are those of gnnmp_lstm_pointwise_f32; equal bits of two calls"""
    import torch
    case = [dev(a) for a in R.lstm_case(N, D)]
    for with_opt in (True, False):
        gx, gh, b, c, dh, dcn = case if with_opt else (case[0], case[1], None, case[3], case[4], None)
        outs = []
        for _ in range(2):
            da, dc = nan(N, 4 * D), nan(N, D)
            assert call_lstm(lib, ptr(gx), ptr(gh), ptr(b), ptr(c), ptr(dh), ptr(dcn), ptr(da), ptr(dc), N, D) == A.OK, lib.gnnmp_last_error()
            torch.cuda.synchronize()
            outs.append((da.cpu().numpy(), dc.cpu().numpy()))
        da_ref, dc_ref = lstm_ref(N, D, 0, with_opt)
        close(outs[0][0], da_ref, "da")
        close(outs[0][1], dc_ref, "dc")
        assert np.array_equal(bits(outs[0][0]), bits(outs[1][0])) and np.array_equal(bits(outs[0][1]), bits(outs[1][1]))


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU 2: the memory contract
# ------------------------------------------------------------------------------------------------------------------------------------
def pool_arrays(D, Dg, seed=0):
    x, sp, q, gate, _, _ = R.pool_case(D, Dg, seed)
    G = len(sp) - 1
    arrs = [A.Arr("x", "in", x), A.Arr("seg_ptr", "in", sp), A.Arr("q", "in", q) if Dg == 0 else A.Arr("gate", "in", gate)]
    return arrs + [A.Arr("r", "out", shape=(G, D)), A.Arr("stats", "out", shape=(G, max(Dg, 1), 2))]


def pool_want(D, Dg, seed=0):
    ref = R.pool_ref(D, Dg, seed)
    return {"r": A.E(ref["r"]), "stats": A.E(ref["stats"])}


def grad_arrays(D, Dg, seed=0, base=None, skip=()):
    """base: None | 'separate' | 'alias' (dx is then an inout array that starts as base)"""
    x, sp, q, gate, dr, b = R.pool_case(D, Dg, seed)
    r, stats = [a.astype(f32) for a in R.pool(x, sp, q, gate)]
    N, G = x.shape[0], len(sp) - 1
    arrs = [A.Arr("dr", "in", dr), A.Arr("x", "in", x), A.Arr("seg_ptr", "in", sp), A.Arr("q", "in", q) if Dg == 0 else A.Arr("gate", "in", gate),
            A.Arr("r", "in", r), A.Arr("stats", "in", stats)]
    if base == "separate":
        arrs.append(A.Arr("base", "in", b))
    outs = [A.Arr("dq", "out", shape=(G, D))] if Dg == 0 else [A.Arr("dgate", "out", shape=(N, Dg))]
    outs.append(A.Arr("dx", "inout", b) if base == "alias" else A.Arr("dx", "out", shape=(N, D)))
    return arrs + [a for a in outs if a.name not in skip]


def grad_want(slab, D, Dg, seed=0, base=None):
    ref = R.pool_ref(D, Dg, seed)
    want = {"dq": ref["dq"], "dgate": ref["dgate"], "dx": ref["dx_base"] if base else ref["dx"]}
    return {k: A.E(v) for k, v in want.items() if k in slab.arrs and slab.arrs[k].role != "in"}


def _p(slab, alias=None):
    alias = alias or {}
    return lambda nm: slab.ptr(alias.get(nm, nm)) if alias.get(nm, nm) in slab.arrs else None


def slab_pool(lib, slab, D, Dg, sp=None):
    p = _p(slab)
    N, G = slab.arrs["x"].shape[0], slab.arrs["seg_ptr"].shape[0] - 1
    return call_pool(lib, p("x"), p("seg_ptr"), p("q"), p("gate"), p("r"), p("stats"), N, G, D, Dg, sp)


def slab_grad(lib, slab, D, Dg, sp=None, base=None):
    p = _p(slab, {"base": "dx"} if base == "alias" else None)
    N, G = slab.arrs["x"].shape[0], slab.arrs["seg_ptr"].shape[0] - 1
    return call_grad(lib, p("dr"), p("x"), p("seg_ptr"), p("q"), p("gate"), p("r"), p("stats"), p("base"), p("dq"), p("dx"), p("dgate"),
                     N, G, D, Dg, sp)


@gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("D", [8, 6, 260])
def test_memory_contract_of_the_segment_exports(lib, D, mode):
    """every element of r, stats, dq, dx, dgate written — the empty segments included — no store before or after an array or into an
    input, with each float array in turn shifted to 16-, 8- and 4-byte alignment (D = 8, 260: 16-byte lanes narrow to 8 and 4; D = 6:
    8-byte lanes narrow to 4), on a side stream; the pullback once per pruned output, with a separate base and with base == dx"""
    import torch
    side = torch.cuda.Stream()
    sp = ctypes.c_void_p(side.cuda_stream)
    Dg = dg_of(mode, D)
    names = [a.name for a in pool_arrays(D, Dg) if a.name != "seg_ptr"]
    for shifts in [{}] + [{nm: A.SHIFTS[a]} for nm in names for a in ("a16", "a8", "a4")]:
        slab = A.Slab(pool_arrays(D, Dg), "cuda", shifts)
        torch.cuda.synchronize()
        rc = slab_pool(lib, slab, D, Dg, sp)
        torch.cuda.synchronize()
        assert rc == A.OK, (shifts, lib.gnnmp_last_error())
        problems = slab.check(pool_want(D, Dg))
        assert not problems, (shifts, problems)
    other = "dq" if mode == "query" else "dgate"
    names = [a.name for a in grad_arrays(D, Dg, base="separate") if a.name != "seg_ptr"]
    runs = [({}, {})] + [({nm: A.SHIFTS[a]}, dict(base="separate")) for nm in names for a in ("a16", "a8", "a4")]
    runs += [({"x": 4}, dict(skip=("dx",))), ({"dr": 8}, dict(skip=(other,))), ({}, dict(base="alias")), ({"dx": 4}, dict(base="alias")),
             ({"dx": 8}, dict(base="alias", skip=(other,)))]
    for shifts, opts in runs:
        slab = A.Slab(grad_arrays(D, Dg, **opts), "cuda", shifts)
        torch.cuda.synchronize()
        rc = slab_grad(lib, slab, D, Dg, sp, opts.get("base"))
        torch.cuda.synchronize()
        assert rc == A.OK, (shifts, opts, lib.gnnmp_last_error())
        problems = slab.check(grad_want(slab, D, Dg, base=opts.get("base")))
        assert not problems, (shifts, opts, problems)


def lstm_arrays(N, D, seed=0):
    names = ("gx", "gh", "b", "c", "dh", "dcn")
    return [A.Arr(nm, "in", a) for nm, a in zip(names, R.lstm_case(N, D, seed))] + [A.Arr("da", "out", shape=(N, 4 * D)),
                                                                                  A.Arr("dc", "out", shape=(N, D))]


def slab_lstm(lib, slab, N, D, sp=None):
    p = _p(slab)
    return call_lstm(lib, p("gx"), p("gh"), p("b"), p("c"), p("dh"), p("dcn"), p("da"), p("dc"), N, D, sp)


@gpu
def test_memory_contract_of_the_lstm_pullback(lib):
    import torch
    N, D = 37, 5
    names = [a.name for a in lstm_arrays(N, D)]
    da, dc = lstm_ref(N, D)
    for shifts in [{}] + [{nm: A.SHIFTS[a]} for nm in names for a in ("a16", "a8", "a4")]:
        slab = A.Slab(lstm_arrays(N, D), "cuda", shifts)
        torch.cuda.synchronize()
        rc = slab_lstm(lib, slab, N, D)
        torch.cuda.synchronize()
        assert rc == A.OK, (shifts, lib.gnnmp_last_error())
        problems = slab.check({"da": A.E(da), "dc": A.E(dc)})
        assert not problems, (shifts, problems)


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU 3: capture
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


def _inputs(arrs):
    return {a.name: a.data for a in arrs if a.role == "in" and a.name != "seg_ptr"}


@gpu
@pytest.mark.parametrize("which", ["pool_query", "pool_all", "grad_query", "grad_one", "lstm"])
def test_the_exports_record_into_a_hip_graph_without_an_eager_call(lib, which):
    D, seeds = 8, (100, 101)
    if which == "lstm":
        N = 19
        slab = A.Slab(lstm_arrays(N, D, seeds[0]))
        call = lambda sp: slab_lstm(lib, slab, N, D, sp)      # noqa: E731
        reloads = [_inputs(lstm_arrays(N, D, sd)) for sd in seeds]
        wants = [dict(zip(("da", "dc"), (A.E(v) for v in lstm_ref(N, D, sd)))) for sd in seeds]
    elif which.startswith("pool"):
        Dg = dg_of(which[5:], D)
        slab = A.Slab(pool_arrays(D, Dg, seeds[0]))
        call = lambda sp: slab_pool(lib, slab, D, Dg, sp)      # noqa: E731
        reloads = [_inputs(pool_arrays(D, Dg, sd)) for sd in seeds]
        wants = [pool_want(D, Dg, sd) for sd in seeds]
    else:
        Dg = dg_of(which[5:], D)
        slab = A.Slab(grad_arrays(D, Dg, seeds[0], base="separate"))
        call = lambda sp: slab_grad(lib, slab, D, Dg, sp)      # noqa: E731
        reloads = [_inputs(grad_arrays(D, Dg, sd, base="separate")) for sd in seeds]
        wants = [grad_want(slab, D, Dg, sd, base="separate") for sd in seeds]
    assert not np.array_equal(list(reloads[0].values())[0], list(reloads[1].values())[0])
    _capture_and_replay(lib, slab, call, reloads, wants)


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU 4: the layers
# ------------------------------------------------------------------------------------------------------------------------------------
def batch_graph(segs=R.SEGS):
    """the batch as a GNNGraph with 0-based indices; the readouts look at its indicator only (one edge, inside the fourth graph)"""
    import gnnmp
    gi = R.indicator(segs, base=0)
    return gnnmp.GNNGraph(dev(np.array([8], np.int64)), dev(np.array([9], np.int64)), num_nodes=len(gi), graph_indicator=dev(gi),
                          num_graphs=len(segs), index_base=0)


def make_set2set(n, iters, Wi, Wh, b, grad=True):
    import gnnmp
    l = gnnmp.Set2Set(n, iters, seed=1)
    l.Wi, l.Wh, l.b = (dev(a).requires_grad_(grad) for a in (Wi, Wh, b))
    return l


def make_chain(chain, grad=True):
    import gnnmp
    layers = []
    for W, b, act in chain:
        d = gnnmp.Dense((W.shape[1], W.shape[0]), act, seed=1)
        d.weight, d.bias = dev(W).requires_grad_(grad), dev(b).requires_grad_(grad)
        layers.append(d)
    return layers


@gpu
@pytest.mark.parametrize("iters", LAYER_ITERS)
@pytest.mark.parametrize("n", LAYER_N)
def test_set2set_ad_against_the_references(n, iters):
    """the forward within 1e-5 of readout_ref, of the oracle and of gnnmp.set2set_pool; dx (accumulated over the iterations through
    base == dx) within 1e-5; dWi, dWh, db by weight_bar.  MEASURED ON THE CPU (test_the_layer_cases_are_well_conditioned prints it): the
    float32 restatement of the reference uses at most 0.0074 of the summation bound γ_n Σ|terms| at one iteration and 0.060 at three
    (n_in = 64, dWi and dWh; 0.0054 at n_in = 3), n = 700, the longest segment, being the longest fold on the path.  The compounded
    reverse-time error stays inside the bound, so weight_bar's fallback (4 x the restatement's own distance) is not taken by these cases.
    With n = 24, the stacked rows of the last fold alone, the restatement itself would read 1.74 of the bound at n_in = 64."""
    import torch
    import gnnmp
    from oracle import more_layers as ML
    x, sp, Wi, Wh, b, dout = R.set2set_case(n)
    ref, rest = R.set2set_ref(n, iters), R.set2set_ref(n, iters, dtype="float32")
    g = batch_graph()
    l = make_set2set(n, iters, Wi, Wh, b)
    xt = dev(x).requires_grad_(True)
    y = gnnmp.set2set_ad(l, g, xt)
    (y * dev(dout)).sum().backward()
    with torch.no_grad():
        old = gnnmp.set2set_pool(l, g, xt)
    torch.cuda.synchronize()
    yn = y.detach().cpu().numpy()
    close(yn, ref["y"], "set2set_ad")
    close(yn, ML.set2set_pool(R.indicator(R.SEGS), len(R.SEGS), x, Wi, Wh, b, iters), "set2set_ad against the oracle")
    close(yn, old.cpu().numpy(), "set2set_ad against set2set_pool")
    close(xt.grad.cpu().numpy(), ref["dx"], "dx")
    for p, k, m in ((l.Wi, "dWi", "mWi"), (l.Wh, "dWh", "mWh"), (l.b, "db", "mb")):
        judge(p.grad.cpu().numpy(), rest[k], ref[k], ref[m], ref["n"], k)


@gpu
@pytest.mark.parametrize("Dg,with_ffeat", R.GAP_VARIANTS)
def test_global_attention_pool_ad_against_the_references(oracle, Dg, with_ffeat):
    """the forward within 1e-5 of readout_ref, of the oracle's composition and of gnnmp.global_attention_pool; dx within 1e-5; every
    weight and bias of fgate and ffeat by weight_bar (n = N = 903 rows)"""
    import torch
    import gnnmp
    from gnnmp.layers_khop import GlobalAttentionPool
    x, sp, fgate, ffeat, dr = R.gap_case(GAP_D, Dg, with_ffeat)
    ref, rest = R.gap_ref(GAP_D, Dg, with_ffeat), R.gap_ref(GAP_D, Dg, with_ffeat, dtype="float32")
    g = batch_graph()
    fg, ff = make_chain(fgate), make_chain(ffeat) if ffeat else None
    l = GlobalAttentionPool(fg, ff)
    xt = dev(x).requires_grad_(True)
    y = gnnmp.global_attention_pool_ad(l, g, xt)
    (y * dev(dr)).sum().backward()

    def run(chain, h):
        for d in chain:
            h = d(h)
        return h
    with torch.no_grad():
        old = gnnmp.global_attention_pool(GlobalAttentionPool(lambda h: run(fg, h), None if ff is None else (lambda h: run(ff, h))), g, xt)
    torch.cuda.synchronize()
    yn = y.detach().cpu().numpy()
    close(yn, ref["y"], "global_attention_pool_ad")
    close(yn, oracle_gap(oracle, x, fgate, ffeat), "global_attention_pool_ad against the oracle")
    close(yn, old.cpu().numpy(), "global_attention_pool_ad against global_attention_pool")
    close(xt.grad.cpu().numpy(), ref["dx"], "dx")
    for name, chain in (("fgate", fg), ("ffeat", ff or [])):
        for k, d in enumerate(chain):
            for p, i, what in ((d.weight, 0, "W"), (d.bias, 1, "b")):
                judge(p.grad.cpu().numpy(), rest[name][k][i], ref[name][k][i], ref[name][k][i + 2], x.shape[0], f"{name}[{k}].{what}")


@gpu
def test_gradients_arrive_only_where_they_are_required():
    """each input alone: its gradient is the full run's (within the 1e-5 bar, not bit for bit: gnnmp_dense_grad_w_f32 sums a bias gradient
    asked for alone by another route), the others stay None; nothing required: no graph is recorded"""
    import torch
    import gnnmp
    from gnnmp.layers_khop import GlobalAttentionPool
    g = batch_graph()
    n, iters = 3, 3
    x, sp, Wi, Wh, b, dout = R.set2set_case(n)

    def s2s(req):
        l = make_set2set(n, iters, Wi, Wh, b, grad=False)
        ts = dict(x=dev(x), Wi=l.Wi, Wh=l.Wh, b=l.b)
        for k in req:
            ts[k].requires_grad_(True)
        y = gnnmp.set2set_ad(l, g, ts["x"])
        if req:
            (y * dev(dout)).sum().backward()
        torch.cuda.synchronize()
        return y, {k: (None if t.grad is None else t.grad.cpu().numpy()) for k, t in ts.items()}
    y, full = s2s(("x", "Wi", "Wh", "b"))
    assert not s2s(())[0].requires_grad
    for k in full:
        _, one = s2s((k,))
        close(one[k], full[k], f"{k} alone")
        assert all(v is None for kk, v in one.items() if kk != k), k
    xg, _, fgate, ffeat, dr = R.gap_case(GAP_D, "all", True)

    def gap(req):
        fg, ff = make_chain(fgate, grad=False), make_chain(ffeat, grad=False)
        ts = dict(x=dev(xg), gW=fg[0].weight, gb=fg[1].bias, fW=ff[0].weight, fb=ff[0].bias)
        for k in req:
            ts[k].requires_grad_(True)
        y = gnnmp.global_attention_pool_ad(GlobalAttentionPool(fg, ff), g, ts["x"])
        if req:
            (y * dev(dr)).sum().backward()
        torch.cuda.synchronize()
        return y, {k: (None if t.grad is None else t.grad.cpu().numpy()) for k, t in ts.items()}
    y, full = gap(("x", "gW", "gb", "fW", "fb"))
    assert not gap(())[0].requires_grad
    for k in full:
        _, one = gap((k,))
        close(one[k], full[k], f"{k} alone")
        assert all(v is None for kk, v in one.items() if kk != k), k


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU 5: one MPNN step
# ------------------------------------------------------------------------------------------------------------------------------------
def mpnn_case():
    """6 graphs of 4 - 9 nodes (ring edges both ways), x [N][4], e [E][3]; NNConv(4 => 5, nn = [Dense(3 => 6, relu), Dense(6 => 20)], relu;
    aggr = mean) -> Set2Set(5, 2 iterations) -> Dense(10 => 2) -> squared error against a target"""
    rng = np.random.default_rng(21)
    ns = (4, 9, 5, 7, 6, 8)
    off = R.ptr_of(ns)
    s = np.concatenate([o + np.r_[np.arange(n), (np.arange(n) + 1) % n] for o, n in zip(off, ns)]).astype(np.int64)
    t = np.concatenate([o + np.r_[(np.arange(n) + 1) % n, np.arange(n)] for o, n in zip(off, ns)]).astype(np.int64)
    N, E, nin, ein, out, hid = int(off[-1]), len(s), 4, 3, 5, 6
    mk = lambda *sh: rng.standard_normal(sh).astype(f32)      # noqa: E731
    nn = [(R.glorot(rng, hid, ein), 0.2 * mk(hid), "relu"), (R.glorot(rng, out * nin, hid), 0.2 * mk(out * nin), None)]
    return dict(ns=ns, s=s, t=t, x=mk(N, nin), e=mk(E, ein), nn=nn, W=R.glorot(rng, out, nin), b=0.2 * mk(out),
                Wi=R.glorot(rng, 4 * out, 2 * out), Wh=R.glorot(rng, 4 * out, out), bl=0.1 * mk(4 * out),
                Wd=R.glorot(rng, 2, 2 * out), bd=0.1 * mk(2), target=mk(len(ns), 2))


def mpnn_model(c, dtype):
    """the step in `dtype` downstream of the NNConv layer (float64 always, tests/nn_conv_ref.py): loss and every gradient"""
    import nn_conv_ref as NR
    ptr_, N = R.ptr_of(c["ns"]), len(c["x"])
    y = NR.compose(c["s"], c["t"], N, c["x"], c["e"], c["nn"], c["W"], c["b"], "relu", "mean")[4]
    Wi, Wh, bl, Wd, bd, target, yd = R.cast(dtype, c["Wi"], c["Wh"], c["bl"], c["Wd"], c["bd"], c["target"], y)
    out, _ = R.set2set(yd, ptr_, Wi, Wh, bl, 2)
    z = out @ Wd.T + bd
    dz = 2 * (z - target)
    s2s = R.set2set_grad(yd, ptr_, Wi, Wh, bl, 2, dz @ Wd)
    conv = NR.grad64(c["s"], c["t"], N, c["x"], c["e"], c["nn"], c["W"], c["b"], "relu", "mean", np.asarray(s2s["dx"], f64))
    return dict(loss=float(((z - target) ** 2).sum()), s2s=s2s, conv=conv, dWd=dz.T @ out, dbd=dz.sum(axis=0), mWd=np.abs(dz).T @ np.abs(out),
                mbd=np.abs(dz).sum(axis=0))


@gpu
def test_one_mpnn_step():
    """nn_conv_ad -> set2set_ad(2 iterations) -> dense_ad -> squared error: every parameter receives a finite gradient; dx, de and the
    NNConv parameters (upstream of the readout, like dx) within 1e-5 of the float64 model built from readout_ref and nn_conv_ref, the
    Set2Set and head parameters by weight_bar; one SGD step of rate 1e-2 lowers the loss"""
    import torch
    import gnnmp
    from gnnmp.backward import dense_ad
    c = mpnn_case()
    ref, rest = mpnn_model(c, f64), mpnn_model(c, f32)
    assert min(float(np.abs(p).min()) for p in ref["conv"]["pres"] + [ref["conv"]["z"]]) >= 1e-4
    gi = R.indicator(c["ns"], base=0)
    g = gnnmp.GNNGraph(dev(c["s"]), dev(c["t"]), num_nodes=len(gi), graph_indicator=dev(gi), num_graphs=len(c["ns"]), index_base=0)
    nn = make_chain(c["nn"])
    conv = gnnmp.NNConv((4, 5), nn, "relu", aggr="mean", seed=1)
    conv.weight, conv.bias = dev(c["W"]).requires_grad_(True), dev(c["b"]).requires_grad_(True)
    s2s = make_set2set(5, 2, c["Wi"], c["Wh"], c["bl"])
    head = make_chain([(c["Wd"], c["bd"], None)])[0]
    xt, et = dev(c["x"]).requires_grad_(True), dev(c["e"]).requires_grad_(True)
    params = [conv.weight, conv.bias, nn[0].weight, nn[0].bias, nn[1].weight, nn[1].bias, s2s.Wi, s2s.Wh, s2s.b, head.weight, head.bias]

    def loss_of():
        z = dense_ad(head, gnnmp.set2set_ad(s2s, g, gnnmp.nn_conv_ad(conv, g, xt, et)))
        return ((z - dev(c["target"])) ** 2).sum()
    loss = loss_of()
    loss.backward()
    torch.cuda.synchronize()
    assert abs(loss.item() - ref["loss"]) <= 1e-5 * ref["loss"]
    for p in params + [xt, et]:
        assert p.grad is not None and bool(torch.isfinite(p.grad).all())
    cv = ref["conv"]
    for got, want, what in ((xt.grad, cv["dx"], "dx"), (et.grad, cv["de"], "de"), (conv.weight.grad, cv["dW"], "dW"), (conv.bias.grad, cv["db"], "db"),
                            (nn[0].weight.grad, cv["nn"][0][0], "nn0.dW"), (nn[0].bias.grad, cv["nn"][0][1], "nn0.db"),
                            (nn[1].weight.grad, cv["nn"][1][0], "nn1.dW"), (nn[1].bias.grad, cv["nn"][1][1], "nn1.db")):
        close(got.cpu().numpy(), want, what)
    rs, ts = ref["s2s"], rest["s2s"]
    for p, k, m in ((s2s.Wi, "dWi", "mWi"), (s2s.Wh, "dWh", "mWh"), (s2s.b, "db", "mb")):
        judge(p.grad.cpu().numpy(), ts[k], rs[k], rs[m], rs["n"], f"Set2Set {k}")
    judge(head.weight.grad.cpu().numpy(), rest["dWd"], ref["dWd"], ref["mWd"], rs["n"], "head dW")      # (the same path: the same n)
    judge(head.bias.grad.cpu().numpy(), rest["dbd"], ref["dbd"], ref["mbd"], rs["n"], "head db")
    with torch.no_grad():
        for p in params:
            p -= 1e-2 * p.grad
        after = loss_of().item()
    print(f"loss {loss.item():.6f} -> {after:.6f}")
    assert after < loss.item()
