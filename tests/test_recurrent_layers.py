"""GConvGRU, GConvLSTM, DCGRU (gnnmp/layers_temporal.py, gnnmp/backward_recurrent.py) and the five exports under them:
gnnmp_poly_hop_ld_f32 (csrc/poly_conv.hip), gnnmp_gru_cell_f32 / gnnmp_gru_cell_grad_f32 / gnnmp_lstm_cell_f32 / gnnmp_lstm_cell_grad_f32
(csrc/recurrent.hip); include/gnnmp.h states the arithmetic, tests/recurrent_ref.py restates cells and kernels.

Without a GPU: the exports exist in header, SYMBOLS and library and take const plans and const host records whose ctypes mirrors have the
header's layout; every refusal comes before any HIP call, by name; empty sizes return OK; one step of each model cell agrees with the same
step composed from oracle.more_layers.cheb_conv / d_conv; the model's gradients pass gradcheck; the layers construct with the reference's
fields and parameter counts; THE CONDITION ON THE INPUTS: the float32 run of the model stays within 2e-6 of float64 for every GPU case.

On the GPU: the panel hop has the hop's bits with every stride = D and is within 1e-5 of float64 on three panels (NaN fill outside the
written block untouched); the gate kernels against float64 with every kind of state; the layers' forward and every gradient within 1e-5
of float64; the per-step launch budget; a training run; one captured training step a layer."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_cases as A  # noqa: E402
import poly_conv_ref as R  # noqa: E402
import recurrent_ref as RR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
gpu = pytest.mark.gpu
f32, f64 = np.float32, np.float64
HOP, GRU, GRUG, LSTM, LSTMG = ("gnnmp_poly_hop_ld_f32", "gnnmp_gru_cell_f32", "gnnmp_gru_cell_grad_f32", "gnnmp_lstm_cell_f32",
                               "gnnmp_lstm_cell_grad_f32")
RECORDS = {HOP: ("gnnmp_poly_hop_ld_t", "PolyHopLdJob"), GRU: ("gnnmp_gru_cell_t", "GruCellJob"), GRUG: ("gnnmp_gru_cell_grad_t", "GruCellGradJob"),
           LSTM: ("gnnmp_lstm_cell_t", "LstmCellJob"), LSTMG: ("gnnmp_lstm_cell_grad_t", "LstmCellGradJob")}
PARAMS = {HOP: ["plan", "job", "D", "stream"], GRU: ["phase", "job", "N", "T", "t", "D", "stream"],
          GRUG: ["phase", "job", "N", "T", "t", "D", "stream"], LSTM: ["job", "N", "T", "t", "D", "stream"],
          LSTMG: ["job", "N", "T", "t", "D", "stream"]}


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
    conventions = header[:header.index("#ifndef GNNMP_H")]
    for name in RECORDS:
        assert f"int {name}(" in header and header.index(f"int {name}(") < internal, name
        assert name in _lib.SYMBOLS and name in exported, name
        assert "} " + RECORDS[name][0] + ";" in header
        assert name in conventions
    assert "tests/test_recurrent_layers.py" in conventions
    for cite in ("temporalconv.jl:237-254", ":416-437", ":564-575"):
        assert cite in header[:internal], cite
    for fn in ("gconv_gru_ad", "gconv_lstm_ad", "dcgru_ad", "GConvGRU", "GConvLSTM", "DCGRU", "GConvGRUCell", "GConvLSTMCell", "DCGRUCell"):
        assert callable(getattr(gnnmp, fn)), fn


@pytest.mark.parametrize("export", list(RECORDS))
def test_the_exports_take_const_plans_and_const_host_records(export):
    """device pointers travel in const host records (the table of tests/abi_cases.py owes no case); the ctypes records have the layout of
    the header's structs: names, offsets, size"""
    from gnnmp import _lib
    decls, _ = A.parse_header()
    assert export not in A.must_be_covered(decls, _lib.SYMBOLS)
    assert [p[0] for p in decls[export]] == PARAMS[export]
    for pname, is_ptr, is_const, _ in decls[export]:
        assert is_const or not is_ptr, pname
    struct, cls = RECORDS[export]
    header = open(os.path.join(ROOT, "include", "gnnmp.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} " + struct + ";", header).group(1)
    body = re.sub(r"/\*.*?\*/", " ", body, flags=re.S)
    fields, off, offsets = [], 0, []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        is_ptr = "*" in decl
        m = re.match(r"^(const\s+)?(float|int64_t|int)\s+(.*)$", decl)
        for nme in [n.strip().lstrip("*").strip() for n in m.group(3).split(",")]:
            size = 8 if (is_ptr or m.group(2) == "int64_t") else 4
            off = (off + size - 1) // size * size
            fields.append(nme)
            offsets.append(off)
            off += size
    rec = getattr(_lib, cls)
    assert tuple(fields) == tuple(f for f, _ in rec._fields_)
    assert [getattr(rec, f).offset for f in fields] == offsets
    assert ctypes.sizeof(rec) == (off + 7) // 8 * 8
    if export == HOP:
        assert [f for f, _ in rec._fields_][:11] == [f for f, _ in _lib.PolyHopJob._fields_]


P_ = lambda v: ctypes.c_void_p(0x1000 * v) if v else None      # never dereferenced: the call must refuse first  # noqa: E731


class _FakePlan(ctypes.Structure):
    """the head of csrc/common.h's gnnmp_graph {int64 n_src, n_dst, n_edges, n_total; ...}: all the refusals read of a plan"""
    _fields_ = [("n_src", ctypes.c_int64), ("n_dst", ctypes.c_int64), ("n_edges", ctypes.c_int64), ("n_total", ctypes.c_int64),
                ("tail", ctypes.c_char * 1024)]


def _hop(lib, plan, job=True, z=1, w_slot=2, ss_slot=3, scale_dst=4, self_=5, prev=6, add=7, out=8, alpha=1.0, beta=0.5, gamma=-1.0, D=4,
         ld=(4, 4, 4, 4, 4), raw=None):
    """pointers are fake pages 0x1000 apart, or raw byte addresses by name in `raw`"""
    from gnnmp import _lib
    raw = raw or {}
    pp = lambda name, v: ctypes.c_void_p(raw[name]) if name in raw else P_(v)      # noqa: E731
    j = _lib.PolyHopLdJob(pp("z", z), P_(w_slot), P_(ss_slot), P_(scale_dst), pp("self", self_), pp("prev", prev), pp("add", add), alpha,
                          beta, gamma, pp("out", out), *ld)
    return lib.gnnmp_poly_hop_ld_f32(plan, ctypes.byref(j) if job else None, D, None)


def _gru(lib, phase=0, job=True, N=5, T=3, t=0, D=4, **kw):
    from gnnmp import _lib
    f = dict(P=1, a=2, h=3, ldh=4, gates=4, hout=5, ldhout=4, rep=1, y=6)
    f.update(kw)
    j = _lib.GruCellJob(P_(f["P"]), P_(f["a"]), P_(f["h"]), f["ldh"], P_(f["gates"]), P_(f["hout"]), f["ldhout"], f["rep"], P_(f["y"]))
    return lib.gnnmp_gru_cell_f32(phase, ctypes.byref(j) if job else None, N, T, t, D, None)


def _grug(lib, phase=1, job=True, N=5, T=3, t=0, D=4, **kw):
    from gnnmp import _lib
    f = dict(dy=1, carry=2, carry2=3, ldc2=4, gates=4, h=5, ldh=4, drh=6, lddrh=4, rep=1, dP=7, dac=8, darz=9, part=10)
    f.update(kw)
    j = _lib.GruCellGradJob(P_(f["dy"]), P_(f["carry"]), P_(f["carry2"]), f["ldc2"], P_(f["gates"]), P_(f["h"]), f["ldh"], P_(f["drh"]),
                            f["lddrh"], f["rep"], P_(f["dP"]), P_(f["dac"]), P_(f["darz"]), P_(f["part"]))
    return lib.gnnmp_gru_cell_grad_f32(phase, ctypes.byref(j) if job else None, N, T, t, D, None)


def _lstm(lib, job=True, N=5, T=3, t=0, D=4, **kw):
    from gnnmp import _lib
    f = dict(P=1, a=2, w=3, c=4, ldc=4, gates=5, cnew=6, hout=7, ldhout=4, y=8)
    f.update(kw)
    j = _lib.LstmCellJob(P_(f["P"]), P_(f["a"]), P_(f["w"]), P_(f["c"]), f["ldc"], P_(f["gates"]), P_(f["cnew"]), P_(f["hout"]), f["ldhout"],
                         P_(f["y"]))
    return lib.gnnmp_lstm_cell_f32(ctypes.byref(j) if job else None, N, T, t, D, None)


def _lstmg(lib, job=True, N=5, T=3, t=0, D=4, **kw):
    from gnnmp import _lib
    f = dict(dy=1, carry_h=2, ldch=4, carry_c=3, gates=4, w=5, c=6, ldc=4, cnew=7, dP=8, da=9, dc=10, peep=11)
    f.update(kw)
    j = _lib.LstmCellGradJob(P_(f["dy"]), P_(f["carry_h"]), f["ldch"], P_(f["carry_c"]), P_(f["gates"]), P_(f["w"]), P_(f["c"]), f["ldc"],
                             P_(f["cnew"]), P_(f["dP"]), P_(f["da"]), P_(f["dc"]), P_(f["peep"]))
    return lib.gnnmp_lstm_cell_grad_f32(ctypes.byref(j) if job else None, N, T, t, D, None)


def test_hop_refusals_need_no_gpu():
    """everything gnnmp_poly_hop_f32 refuses, a stride below D, and the aliasing rules — under the export's own name, before any HIP call"""
    from gnnmp import _lib
    lib = _lib.load()
    E, err = _lib.EINVAL, lib.gnnmp_last_error
    sq = _FakePlan(n_src=5, n_dst=5, n_edges=7, n_total=7)
    pl = ctypes.addressof(sq)
    assert _hop(lib, None) == E and b"poly_hop_ld: null plan" in err()
    assert _hop(lib, pl, job=False) == E and b"poly_hop_ld: null job" in err()
    assert _hop(lib, pl, z=None) == E and b"poly_hop_ld: null z" in err()
    assert _hop(lib, pl, out=None) == E and b"poly_hop_ld: null out" in err()
    for D in (0, -1, (1 << 19) + 1, 2 ** 40):
        assert _hop(lib, pl, D=D, ld=(2 ** 40,) * 5) == E and b"poly_hop_ld: bad D" in err(), D
    for k, nm in enumerate(("ld_z", "ld_self", "ld_prev", "ld_add", "ld_out")):
        ld = [4] * 5
        ld[k] = 3
        assert _hop(lib, pl, ld=tuple(ld)) == E and b"poly_hop_ld: " + nm.encode() in err() and b"below D" in err(), nm
    # the stride of a NULL operand is not read: the call gets as far as the refusal that follows the stride checks
    assert _hop(lib, pl, self_=None, prev=None, add=None, ld=(4, 0, 0, 0, 4)) == E and b"beta != 0 with a null self" in err()
    assert _hop(lib, pl, out=1) == E and b"poly_hop_ld: out overlaps z" in err()
    assert _hop(lib, pl, out=5) == E and b"poly_hop_ld: out overlaps self" in err()
    assert _hop(lib, pl, self_=None) == E and b"poly_hop_ld: beta != 0 with a null self" in err()
    assert _hop(lib, pl, prev=None) == E and b"poly_hop_ld: gamma != 0 with a null prev" in err()
    # blocks of one panel [5][12], D = 4: block 0 = z and self, block 1 = prev and out, block 2 = add — distinct blocks are allowed
    base = 0x100000
    blk = lambda j: base + 16 * j      # noqa: E731
    ok = dict(z=blk(0), self=blk(0), prev=blk(1), add=blk(2), out=blk(1))
    # (the allowed layouts are shown to pass the overlap checks by the refusal that comes AFTER them: no call here may reach a launch)
    noself = {k: v for k, v in ok.items() if k != "self"}
    assert _hop(lib, pl, ld=(12,) * 5, raw=noself, self_=None) == E and b"beta != 0 with a null self" in err()                               # out = prev
    assert _hop(lib, pl, ld=(12,) * 5, raw=dict(noself, prev=blk(2), add=blk(1)), self_=None) == E and b"beta != 0 with a null self" in err()  # out = add
    assert _hop(lib, pl, ld=(12,) * 5, raw=dict(ok, out=blk(0), prev=blk(0))) == E and b"out overlaps z" in err()
    assert _hop(lib, pl, ld=(12,) * 5, raw=dict(ok, out=blk(0) + 8)) == E and b"out overlaps z" in err()           # half a block in
    assert _hop(lib, pl, ld=(12,) * 5, raw=dict(ok, z=blk(2), out=blk(0))) == E and b"out overlaps self" in err()
    assert _hop(lib, pl, ld=(12, 12, 16, 12, 12), raw=ok) == E and b"out overlaps prev without being it" in err()  # same pointer, other stride
    assert _hop(lib, pl, ld=(12, 12, 12, 16, 12), raw=dict(ok, add=blk(1))) == E and b"out overlaps add without being it" in err()
    assert _hop(lib, pl, ld=(12,) * 5, raw=dict(ok, add=blk(1) + 4)) == E and b"out overlaps add" in err()


def test_cell_refusals_need_no_gpu():
    from gnnmp import _lib
    lib = _lib.load()
    E, err = _lib.EINVAL, lib.gnnmp_last_error
    for fn, who, extra in ((_gru, b"gru_cell", {}), (_grug, b"gru_cell_grad", {}), (_lstm, b"lstm_cell", None), (_lstmg, b"lstm_cell_grad", None)):
        assert fn(lib, job=False) == E and who + b": null job" in err()
        assert fn(lib, N=-1) == E and who + b": negative N" in err()
        for D in (0, -3, (1 << 20) + 1):
            assert fn(lib, D=D) == E and who + b": bad D" in err(), D
        for T in (0, (1 << 20) + 1):
            assert fn(lib, T=T) == E and who + b": bad T" in err(), T
        for t in (-1, 3):
            assert fn(lib, t=t) == E and who + b": step" in err(), t
        if extra is not None:
            assert fn(lib, phase=2) == E and who + b": bad phase" in err()
            assert fn(lib, rep=3) == E and who + b": bad rep" in err()
    for nm in ("P", "a", "gates"):
        assert _gru(lib, **{nm: None}) == E and b"gru_cell: null P, a or gates" in err(), nm
    assert _gru(lib, 0, hout=None) == E and b"gru_cell: null hout in phase 0" in err()
    assert _gru(lib, 1, y=None) == E and b"gru_cell: null y in phase 1" in err()
    assert _gru(lib, ldh=3) == E and b"gru_cell: stride of h" in err()
    assert _gru(lib, ldhout=3) == E and b"gru_cell: ldhout" in err()
    assert _gru(lib, rep=2, ldhout=7) == E and b"gru_cell: ldhout" in err()
    for nm in ("gates", "dP", "darz", "part"):
        assert _grug(lib, **{nm: None}) == E and b"gru_cell_grad: null gates, dP, darz or part" in err(), nm
    for nm in ("dy", "dac"):
        assert _grug(lib, 1, **{nm: None}) == E and b"gru_cell_grad: null dy or dac in phase 1" in err(), nm
    assert _grug(lib, 0, drh=None) == E and b"gru_cell_grad: null drh in phase 0" in err()
    assert _grug(lib, ldh=2) == E and b"gru_cell_grad: stride of h" in err()
    assert _grug(lib, 1, ldc2=3) == E and b"gru_cell_grad: ldc2" in err()
    assert _grug(lib, 0, lddrh=3) == E and b"gru_cell_grad: lddrh" in err()
    for nm in ("P", "a", "w"):
        assert _lstm(lib, **{nm: None}) == E and b"lstm_cell: null P, a or w" in err(), nm
    for nm in ("gates", "cnew", "y"):
        assert _lstm(lib, **{nm: None}) == E and b"lstm_cell: null gates, cnew or y" in err(), nm
    assert _lstm(lib, ldc=1) == E and b"lstm_cell: stride of c" in err()
    assert _lstm(lib, ldhout=3) == E and b"lstm_cell: ldhout" in err()
    for nm in ("dy", "gates", "w", "cnew"):
        assert _lstmg(lib, **{nm: None}) == E and b"lstm_cell_grad: null dy, gates, w or cnew" in err(), nm
    for nm in ("dP", "da", "dc"):
        assert _lstmg(lib, **{nm: None}) == E and b"lstm_cell_grad: null dP, da or dc" in err(), nm
    assert _lstmg(lib, ldc=3) == E and b"lstm_cell_grad: stride of c" in err()
    assert _lstmg(lib, ldch=3) == E and b"lstm_cell_grad: ldch" in err()


def test_empty_sizes_return_ok_without_a_device():
    from gnnmp import _lib
    lib = _lib.load()
    for plan in (_FakePlan(n_src=0, n_dst=0, n_edges=0, n_total=0), _FakePlan(n_src=9, n_dst=0, n_edges=0, n_total=0)):
        pn = ctypes.addressof(plan)
        assert _hop(lib, pn) == _lib.OK
        assert _hop(lib, pn, w_slot=None, ss_slot=None, scale_dst=None, self_=None, prev=None, add=None, beta=0.0, gamma=0.0) == _lib.OK
        assert _hop(lib, pn, out=6) == _lib.OK and _hop(lib, pn, out=7) == _lib.OK      # out = prev, out = add
    for phase in (0, 1):
        assert _gru(lib, phase, N=0) == _lib.OK and _gru(lib, phase, N=0, h=None, D=1 << 20, ldhout=1 << 20) == _lib.OK
        assert _grug(lib, phase, N=0) == _lib.OK and _grug(lib, phase, N=0, h=None, carry=None, carry2=None) == _lib.OK
    assert _gru(lib, 1, N=0, hout=None) == _lib.OK and _gru(lib, 0, N=0, ldh=0) == _lib.OK
    assert _lstm(lib, N=0) == _lib.OK and _lstm(lib, N=0, c=None, hout=None) == _lib.OK and _lstm(lib, N=0, ldc=0) == _lib.OK
    assert _lstmg(lib, N=0) == _lib.OK and _lstmg(lib, N=0, c=None, carry_h=None, carry_c=None, peep=None) == _lib.OK


# ------------------------------------------------------------------------------------------------------------------------------------
# CPU: the model
# ------------------------------------------------------------------------------------------------------------------------------------
def _close64(got, ref, tol=1e-5):
    got, ref = np.asarray(got, f64), np.asarray(ref, f64)
    return np.linalg.norm(got - ref) <= tol * np.linalg.norm(ref) and np.abs(got - ref).max() <= tol * np.abs(ref).max()


def test_the_torch_hop_is_the_numpy_hop():
    """recurrent_ref.hop is poly_conv_ref.hop statement by statement: equal to rounding in float64 on the multigraph, every operand on"""
    import torch
    s, t, ops = R.hop_case(7, False)
    want = R.hop_ref(7, False, (True,) * 6)
    tt = lambda a: torch.from_numpy(a.astype(f64))      # noqa: E731
    got = RR.hop(torch.from_numpy(s), torch.from_numpy(t), R.N_NODES, tt(ops["z"]), tt(ops["w"]), tt(ops["ss"]), tt(ops["sd"]), R.ALPHA, R.BETA,
                 tt(ops["self_"]), R.GAMMA, tt(ops["prev"]), tt(ops["add"])).numpy()
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


def _first(kind, gname):
    """the case of the highest order on that graph"""
    return max((c for c in RR.LAYER_CASES if c[0] == kind and c[1] == gname and c[6] == RR.OUT), key=lambda c: c[2])


@pytest.mark.parametrize("kind,gname", [("gconv_gru", "bi"), ("gconv_gru", "bi_w"), ("gconv_lstm", "bi"), ("dcgru", "di_w"), ("dcgru", "ring")])
def test_one_model_step_agrees_with_the_oracle_composed_as_the_reference(kind, gname):
    """one step of each cell in recurrent_ref (float64) against the same step composed from oracle.more_layers.cheb_conv / d_conv calls
    exactly as temporalconv.jl composes it, at 1e-5"""
    import torch
    from oracle import more_layers as ML
    c = _first(kind, gname)
    k = c[2]
    s, t, n, w, _ = RR.graph_of(gname)
    case = RR.layer_case(c)
    p = case["params"]
    x = case["x"][:, 0]
    rng = np.random.default_rng(5)
    h = (0.5 * rng.standard_normal((n, RR.OUT))).astype(f32)
    cc = (0.5 * rng.standard_normal((n, RR.OUT))).astype(f32)
    sig = lambda v: np.where(v >= 0, 1 / (1 + np.exp(-np.abs(v))), np.exp(-np.abs(v)) / (1 + np.exp(-np.abs(v))))      # noqa: E731
    cheb = lambda v, W, b: ML.cheb_conv(s + 1, t + 1, n, v, W, b, k, edge_weight=w).astype(f64)      # noqa: E731
    dconv = lambda v, W, b: ML.d_conv(s + 1, t + 1, n, v, W, b, k, edge_weight=w).astype(f64)      # noqa: E731
    G = RR.Graph(s, t, n, w, None if kind == "dcgru" else RR.lam_of(gname))
    tp = [None if a is None else torch.from_numpy(a).double() for a in p]
    tx, th, tc = torch.from_numpy(x).double(), torch.from_numpy(h).double(), torch.from_numpy(cc).double()
    if kind == "gconv_gru":
        r = sig(cheb(x, p[0], p[1]) + cheb(h, p[2], p[3]))
        z = sig(cheb(x, p[4], p[5]) + cheb(h, p[6], p[7]))
        ht = np.tanh(cheb(x, p[8], p[9]) + cheb((r * h).astype(f32), p[10], p[11]))
        want = (1 - z) * ht + z * h
        got = RR.gconv_gru_cell(G, tp, tx, th)[0].numpy()
    elif kind == "gconv_lstm":
        zero = np.zeros(RR.OUT, f32)
        pre = lambda q, cv: cheb(x, p[6 * q], p[6 * q + 1]) + cheb(h, p[6 * q + 2], p[6 * q + 3]) + p[6 * q + 4] * cv + (zero if p[6 * q + 5] is None else p[6 * q + 5])      # noqa: E731
        i, f = sig(pre(0, cc)), sig(pre(1, cc))
        cn = f * cc + i * np.tanh(pre(2, cc))
        o = sig(pre(3, cn))
        want = o * np.tanh(cn)
        got, (_, gc) = RR.gconv_lstm_cell(G, tp, tx, (th, tc))
        got = got.numpy()
        assert _close64(gc.numpy(), cn)
    else:
        xh = np.concatenate([x, h], 1)
        z, r = sig(dconv(xh, p[0], p[1])), sig(dconv(xh, p[2], p[3]))
        cand = np.tanh(dconv(np.concatenate([x, (h * r).astype(f32)], 1), p[4], p[5]))
        want = z * h + (1 - z) * cand
        got = RR.dcgru_cell(G, tp, tx, th)[0].numpy()
    assert _close64(got, want), RR.rel(got, want)


@pytest.mark.parametrize("kind", ["gconv_gru", "gconv_lstm", "dcgru"])
def test_the_model_gradients_pass_gradcheck(kind):
    """torch.autograd.gradcheck of the scan in float64 on the smallest case: k = 2, T = 2, 6 nodes, 2 => 3 channels"""
    import torch
    n = 6
    if kind == "dcgru":                                      # a directed 6-ring with two chords
        G = RR.Graph(np.array([0, 1, 2, 3, 4, 5, 0, 2]), np.array([1, 2, 3, 4, 5, 0, 3, 5]), n)
    else:                                                    # the bidirected 6-ring with one chord; λmax is a constant of the graph
        s, t = np.array([0, 1, 2, 3, 4, 5, 0]), np.array([1, 2, 3, 4, 5, 0, 3])
        G = RR.Graph(np.concatenate([s, t]), np.concatenate([t, s]), n, None, 1.9)
    gen = torch.Generator().manual_seed(3)
    rn = lambda *sh: (0.5 * torch.randn(sh, generator=gen, dtype=torch.float64)).requires_grad_()      # noqa: E731
    cin, out, k, T = 2, 3, 2, 2
    if kind == "dcgru":
        p = [q for _ in range(3) for q in (rn(2, k, out, cin + out), rn(out))]
    else:
        p = []
        for _ in range(3 if kind == "gconv_gru" else 4):
            p += [rn(k, out, cin), rn(out), rn(k, out, out), rn(out)] + ([rn(out), rn(out)] if kind == "gconv_lstm" else [])
    x, h, c = rn(n, T, cin), rn(n, out), rn(n, out)

    def fn(x_, h_, c_, *p_):
        return RR.scan(kind, G, list(p_), x_, (h_, c_) if kind == "gconv_lstm" else h_)
    assert torch.autograd.gradcheck(fn, (x, h, c, *p), eps=1e-6, atol=1e-6, rtol=1e-5)


def test_the_layers_construct_with_the_reference_fields_and_parameter_counts():
    """GConvGRUCell(2 => 3, 2): 108 parameters, GConvLSTMCell(2 => 3, 2): 168, DCGRUCell(2 => 3, 2): 189 (temporalconv.jl's docstrings)"""
    import gnnmp
    count = lambda cell: sum(int(p.numel()) for p in cell.parameters() if p is not None)      # noqa: E731
    gru = gnnmp.GConvGRUCell((2, 3), 2, device="cpu")
    assert count(gru) == 108 and len(gru.parameters()) == 12
    for n in ("conv_x_r", "conv_h_r", "conv_x_z", "conv_h_z", "conv_x_h", "conv_h_h"):
        conv = getattr(gru, n)
        assert isinstance(conv, gnnmp.ChebConv) and tuple(conv.weight.shape) == (2, 3, 2 if "_x_" in n else 3) and tuple(conv.bias.shape) == (3,)
    assert (gru.k, gru.in_, gru.out) == (2, 2, 3) and tuple(gru.initialstates().shape) == (3,)
    lstm = gnnmp.GConvLSTMCell((2, 3), 2, device="cpu")
    assert count(lstm) == 168 and len(lstm.parameters()) == 24
    for q in "ifco":
        assert isinstance(getattr(lstm, "conv_x_" + q), gnnmp.ChebConv) and isinstance(getattr(lstm, "conv_h_" + q), gnnmp.ChebConv)
        assert tuple(getattr(lstm, "w_" + q).shape) == (3,) and tuple(getattr(lstm, "b_" + q).shape) == (3,)
    assert all(tuple(v.shape) == (3,) for v in lstm.initialstates())
    dc = gnnmp.DCGRUCell((2, 3), 2, device="cpu")
    assert count(dc) == 189 and len(dc.parameters()) == 6
    for n in ("dconv_u", "dconv_r", "dconv_c"):
        d = getattr(dc, n)
        assert isinstance(d, gnnmp.DConv) and tuple(d.weights.shape) == (2, 2, 3, 5) and tuple(d.bias.shape) == (3,)
    assert (dc.k, dc.in_, dc.out) == (2, 2, 3)
    nob = gnnmp.GConvLSTMCell((2, 3), 2, bias=False, device="cpu")
    assert nob.b_i is None and nob.conv_x_i.bias is None and count(nob) == 168 - 4 * 9
    for make in (gnnmp.GConvGRU, gnnmp.GConvLSTM, gnnmp.DCGRU):
        layer = make((2, 3), 2, device="cpu")
        assert isinstance(layer, gnnmp.GNNRecurrence) and layer.cell.k == 2
        with pytest.raises(ValueError, match="k must be at least 1"):
            make((2, 3), 0, device="cpu")
        with pytest.raises(ValueError, match="channels must be positive"):
            make((0, 3), 2, device="cpu")


def test_the_generic_scan_takes_the_cell_result_in_the_reference_order():
    """GNNRecurrence's generic loop unpacks (output, state): a cell with a pair state scans correctly"""
    import gnnmp
    import torch

    class Pair:
        def __call__(self, g, x, state):
            h, c = state
            return x + h, (h + 1, c)
    y = gnnmp.GNNRecurrence(Pair())(None, torch.zeros(2, 3, 1), (torch.zeros(2, 1), None))
    assert y[:, :, 0].tolist() == [[0.0, 1.0, 2.0]] * 2


@pytest.mark.parametrize("c", RR.LAYER_CASES, ids=RR.case_id)
def test_the_layer_cases_are_well_conditioned(c):
    """THE CONDITION ON THE INPUTS, not a measurement: the float32 run of the model is within 2e-6, norm-wise, of its float64 run, for y
    and every gradient, for every case used on the GPU"""
    worst = RR.layer_condition(c)
    assert worst <= RR.COND, f"the float32 run is {worst:.2e} from float64 (bound {RR.COND:g})"


@pytest.mark.parametrize("N", RR.GATE_NS)
@pytest.mark.parametrize("D", RR.GATE_DS)
def test_the_gate_cases_are_well_conditioned(D, N):
    """the header's formulas in float32 numpy within 2e-6 of float64 for every output the GPU tests compare, every kind of state, both
    steps (N = 1, D = 1 is ONE element: no other element hides a cancellation there)"""
    for kind in RR.H_KINDS:
        for t in RR.GATE_TS:
            assert RR.gate_condition("gru", N, D, t, kind) <= RR.COND, ("gru", kind, t)
            assert RR.gate_condition("lstm", N, D, t, kind) <= RR.COND, ("lstm", kind, t)


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU helpers
# ------------------------------------------------------------------------------------------------------------------------------------
def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def tbits(t):
    return bits(t.detach().cpu().numpy())


def close(got, ref, what, tol=1e-5):
    """the project's parity bar, norm-wise AND element-wise against the array scale"""
    import torch
    if isinstance(got, torch.Tensor):
        got = got.detach().cpu().numpy()
    got, ref = np.asarray(got, f64), np.asarray(ref, f64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.all(np.isfinite(got)), f"{what}: non-finite"
    err, scale = np.linalg.norm(got - ref), np.linalg.norm(ref)
    worst = np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300) if ref.size else 0.0
    print(f"{what}: |got - ref| = {err:.3e}, |ref| = {scale:.3e}, ratio {err / max(scale, 1e-300):.2e}, element-wise {worst:.2e}")
    assert err <= tol * scale, f"{what}: {err:.3e} > {tol:g} * {scale:.3e}"
    assert worst <= tol, f"{what}: element-wise {worst:.2e} of the array scale"


def ptr(v, off=0):
    return None if v is None else ctypes.c_void_p(v.data_ptr() + 4 * off)


def nan(*shape):
    import torch
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


@pytest.fixture(scope="module")
def lib():
    import torch
    assert torch.cuda.is_available()
    from gnnmp import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def graph(lib):
    import gnnmp
    s, t, tie = R.graph()
    g = gnnmp.GNNGraph(dev(s), dev(t), num_nodes=R.N_NODES, index_base=0)
    g.plan(False), g.plan_transposed(False)
    return g


NAMES = dict(zip(R.FIELDS, ("w_slot", "ss_slot", "scale_dst", "self", "prev", "add")))
HOP_COMBOS = [(True,) * 6, (False,) * 6, (True, False, True, False, True, False), (False, True, False, True, False, True),
              (True, True, False, True, True, False), (False, False, True, False, False, True)]


def slot_arrays(s, t, ops, combo):
    order = np.argsort(t, kind="stable")
    arrs = {"z": ops["z"]}
    for k, on in zip(R.FIELDS, combo):
        if on:
            arrs[NAMES[k]] = ops[k][order] if k in ("w", "ss") else ops[k]
    return arrs


def coeffs(combo):
    on = dict(zip(R.FIELDS, combo))
    return R.ALPHA, R.BETA if on["self_"] else 0.0, R.GAMMA if on["prev"] else 0.0


def call_hop_ld(lib, plan, p, ld, alpha, beta, gamma, D, stream=None, out="out"):
    """p(name) -> pointer | None; ld(name) -> stride"""
    from gnnmp import _lib
    job = _lib.PolyHopLdJob(p("z"), p("w_slot"), p("ss_slot"), p("scale_dst"), p("self"), p("prev"), p("add"), alpha, beta, gamma, p(out),
                            ld("z"), ld("self"), ld("prev"), ld("add"), ld(out))
    return lib.gnnmp_poly_hop_ld_f32(plan, ctypes.byref(job), D, stream)


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU 1: the panel hop
# ------------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("transposed", [False, True], ids=["plan", "plan_t"])
@pytest.mark.parametrize("D", R.WIDTHS)
def test_hop_ld_with_every_stride_D_has_the_bits_of_the_hop(lib, graph, D, transposed):
    """the shared kernel template launched from both exports: equal bits over the plan and the transposed plan of the multigraph (hub rows,
    a row without slots) at every lane width"""
    import torch
    from gnnmp import _lib
    s, t, ops = R.hop_case(D, transposed)
    plan = (graph.plan_transposed(False) if transposed else graph.plan(False)).handle
    for combo in HOP_COMBOS:
        held = {k: dev(v) for k, v in slot_arrays(s, t, ops, combo).items()}
        a, b, c = coeffs(combo)
        want, got = nan(R.N_NODES, D), nan(R.N_NODES, D)
        p = lambda nm: ptr(held.get(nm))      # noqa: E731
        job = _lib.PolyHopJob(p("z"), p("w_slot"), p("ss_slot"), p("scale_dst"), p("self"), p("prev"), p("add"), a, b, c, ptr(want))
        assert lib.gnnmp_poly_hop_f32(plan, ctypes.byref(job), D, None) == A.OK, lib.gnnmp_last_error()
        held["out"] = got
        assert call_hop_ld(lib, plan, p, lambda nm: D, a, b, c, D) == A.OK, lib.gnnmp_last_error()
        torch.cuda.synchronize()
        assert np.array_equal(tbits(got), tbits(want)), combo
        close(got, R.hop_ref(D, transposed, combo), f"hop_ld {combo}")


# (D, panel row stride, column offsets of z / self, prev, add, out): 16-byte lanes; an odd stride; an even stride with odd block offsets
PANELS = [(8, 48, dict(z=0, prev=8, add=16, out=24)), (8, 45, dict(z=0, prev=8, add=16, out=24)), (6, 40, dict(z=1, prev=9, add=17, out=25)),
          (260, 1100, dict(z=4, prev=268, add=532, out=796))]


@gpu
@pytest.mark.parametrize("alias", [None, "prev", "add"])
@pytest.mark.parametrize("transposed", [False, True], ids=["plan", "plan_t"])
@pytest.mark.parametrize("D,ld,cols", PANELS, ids=["vec4", "odd_stride", "odd_offset", "two_tiles"])
def test_hop_ld_on_panels(lib, graph, D, ld, cols, transposed, alias):
    """z (= self), prev, add and out as column blocks of ONE allocation [N][ld] filled with NaN: out within 1e-5 of float64, norm-wise and
    element-wise; the inputs and every column outside the written block keep their bits; out = prev and out = add give the bits of the call
    with a block of its own; two calls give equal bits"""
    import torch
    s, t, ops = R.hop_case(D, transposed)
    plan = (graph.plan_transposed(False) if transposed else graph.plan(False)).handle
    combo = (True,) * 6
    arrs = slot_arrays(s, t, ops, combo)
    a, b, c = coeffs(combo)
    ref = R.hop_ref(D, transposed, combo)
    N = R.N_NODES

    def run(alias=alias):
        panel = nan(N, ld)
        for nm in ("z", "prev", "add"):
            panel[:, cols[nm]:cols[nm] + D] = dev(arrs[nm])
        # self lives in an allocation of its own, with its own stride D: the strides of one call need not agree
        side = {k: dev(arrs[k]) for k in ("w_slot", "ss_slot", "scale_dst", "self")}
        before = panel.clone()
        col = dict(cols, out=cols[alias] if alias else cols["out"])
        p = lambda nm: ptr(side[nm]) if nm in side else ptr(panel, col[nm])      # noqa: E731
        rc = call_hop_ld(lib, plan, p, lambda nm: D if nm == "self" else ld, a, b, c, D)
        assert rc == A.OK, lib.gnnmp_last_error()
        torch.cuda.synchronize()
        return panel, before, col["out"]
    panel, before, oc = run()
    got = panel[:, oc:oc + D]
    close(got, ref, f"hop_ld on a panel (D = {D}, ld = {ld})")
    keep = np.ones(ld, bool)
    keep[oc:oc + D] = False
    assert np.array_equal(tbits(panel)[:, keep], tbits(before)[:, keep]), "a column outside the written block changed"
    again, _, _ = run()
    assert np.array_equal(tbits(again), tbits(panel))
    if alias:
        sep, _, soc = run(None)
        assert np.array_equal(tbits(got), tbits(sep[:, soc:soc + D])), alias


@gpu
def test_hop_ld_with_self_as_the_z_block(lib, graph):
    """cheb_conv's call: self IS z (one block), prev another block, out a third — the layers' first two orders on one panel"""
    import torch
    D, ld = 6, 24
    s, t, ops = R.hop_case(D, False)
    plan = graph.plan(False).handle
    panel = nan(R.N_NODES, ld)
    panel[:, 0:D], panel[:, D:2 * D] = dev(ops["z"]), dev(ops["prev"])
    col = dict(z=0, self=0, prev=D, out=2 * D)
    rc = call_hop_ld(lib, plan, lambda nm: ptr(panel, col[nm]) if nm in col else None, lambda nm: ld, R.ALPHA, R.BETA, R.GAMMA, D)
    assert rc == A.OK, lib.gnnmp_last_error()
    torch.cuda.synchronize()
    ref = R.hop(s, t, R.N_NODES, ops["z"].astype(f64), alpha=R.ALPHA, beta=R.BETA, self_=ops["z"].astype(f64), gam=R.GAMMA,
                prev=ops["prev"].astype(f64))
    close(panel[:, 2 * D:3 * D], ref, "hop_ld with self = z")
    assert bool(torch.isnan(panel[:, 3 * D:]).all())


@gpu
@pytest.mark.parametrize("transposed", [False, True], ids=["plan", "plan_t"])
def test_hop_ld_records_into_a_hip_graph_without_an_eager_call(lib, transposed):
    """a fresh plan, no eager call first; capture_error_mode thread_local: an allocation or a host wait would fail the capture; the replay
    has the eager call's bits, also on new values"""
    import torch
    D, ld = 8, 48
    cols = dict(z=0, prev=8, add=16, out=24)
    s0, t0, _ = R.graph()
    g = A.Graph("poly_ld", s0 + 1, t0 + 1, R.N_NODES)
    plans = A.Plans(lib)
    try:
        plan = plans.get(A.Pl(g, T=transposed))
        combo = (True,) * 6
        a, b, c = coeffs(combo)
        panel = nan(R.N_NODES, ld)
        side = {}

        def load(seed):
            s, t, ops = R.hop_case(D, transposed, seed)
            arrs = slot_arrays(s, t, ops, combo)
            with torch.no_grad():
                panel.fill_(float("nan"))
                for nm in ("z", "prev", "add"):
                    panel[:, cols[nm]:cols[nm] + D] = dev(arrs[nm])
                for k in ("w_slot", "ss_slot", "scale_dst", "self"):
                    if k in side:
                        side[k].copy_(dev(arrs[k]))
                    else:
                        side[k] = dev(arrs[k])
        load(100)
        p = lambda nm: ptr(side[nm]) if nm in side else ptr(panel, cols[nm])      # noqa: E731
        stream = torch.cuda.Stream()
        sp = ctypes.c_void_p(stream.cuda_stream)
        graph_ = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            graph_.capture_begin(capture_error_mode="thread_local")
            try:
                rc = call_hop_ld(lib, plan, p, lambda nm: D if nm == "self" else ld, a, b, c, D, sp)
            finally:
                graph_.capture_end()
        torch.cuda.synchronize()
        assert rc == A.OK, lib.gnnmp_last_error()
        assert bool(torch.isnan(panel[:, 24:32]).all()), "work ran while the call was being recorded"
        for seed in (100, 101):
            load(seed)
            graph_.replay()
            torch.cuda.synchronize()
            rep = tbits(panel)
            close(panel[:, 24:32], R.hop_ref(D, transposed, combo, seed), f"replayed hop_ld, seed {seed}")
            load(seed)
            assert call_hop_ld(lib, plan, p, lambda nm: D if nm == "self" else ld, a, b, c, D, sp) == A.OK
            torch.cuda.synchronize()
            assert np.array_equal(tbits(panel), rep)
        del graph_
    finally:
        plans.close()


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU 2: the gate kernels
# ------------------------------------------------------------------------------------------------------------------------------------
def _state_dev(ops, kind):
    """(tensor | None, stride) of a state of the given kind; 'mat' sits in a wider NaN panel at an odd column so that the stride is used"""
    if kind == "null":
        return None, 0, 0
    if kind == "vec":
        return dev(ops["hvec"]), 0, 0
    N, D = ops["h"].shape
    pan = nan(N, 2 * D + 3)
    pan[:, 3:3 + D] = dev(ops["h"])
    return pan, 2 * D + 3, 3


def _gru_run(lib, ops, hkind, t, rep, N, D, stream=None, with_hout1=True):
    """both phases of the forward, then both of the pullback; returns the device tensors"""
    from gnnmp import _lib
    T = RR.GATE_T
    h, ldh, hoff = _state_dev(ops, hkind)
    hp = ptr(h, hoff)
    P = dev(ops["P"])
    a0, a1 = dev(ops["a"][:, :2 * D]), dev(ops["a"][:, 2 * D:])
    gates, y = nan(N, T, 3 * D), nan(N, T, D)
    ldo = rep * D + 5
    rh, hn = nan(N, ldo), nan(N, ldo)
    job = _lib.GruCellJob(ptr(P), ptr(a0), hp, ldh, ptr(gates), ptr(rh, 2), ldo, rep, None)
    assert lib.gnnmp_gru_cell_f32(0, ctypes.byref(job), N, T, t, D, stream) == A.OK, lib.gnnmp_last_error()
    job = _lib.GruCellJob(ptr(P), ptr(a1), hp, ldh, ptr(gates), ptr(hn, 2) if with_hout1 else None, ldo, rep, ptr(y))
    assert lib.gnnmp_gru_cell_f32(1, ctypes.byref(job), N, T, t, D, stream) == A.OK, lib.gnnmp_last_error()
    out = dict(gates=gates, y=y, rh=rh, hn=hn, keep=(P, a0, a1, h))
    return out


def _gru_grad_run(lib, ops, fwd, hkind, t, rep, carries, N, D, stream=None):
    from gnnmp import _lib
    T = RR.GATE_T
    h = fwd["keep"][3]
    ldh, hoff = (0, 0) if hkind != "mat" else (2 * D + 3, 3)
    hp = ptr(h, hoff)
    dy = dev(ops["dy"])
    carry = dev(ops["carry"]) if carries[0] else None
    c2 = nan(N, 2 * D + 1)
    c2[:, 1:1 + rep * D] = dev(ops["carry2"][:, :rep * D])
    drh = nan(N, 2 * D + 1)
    drh[:, 1:1 + rep * D] = dev(ops["drh"][:, :rep * D])
    dP, dac, darz, part = nan(N, T, 3 * D), nan(N, D), nan(N, 2 * D), nan(N, D)
    job = _lib.GruCellGradJob(ptr(dy), ptr(carry), ptr(c2, 1) if carries[1] else None, 2 * D + 1, ptr(fwd["gates"]), hp, ldh, None, 2 * D + 1,
                              rep, ptr(dP), ptr(dac), ptr(darz), ptr(part))
    assert lib.gnnmp_gru_cell_grad_f32(1, ctypes.byref(job), N, T, t, D, stream) == A.OK, lib.gnnmp_last_error()
    import torch
    torch.cuda.synchronize()
    part1 = part.clone()
    job = _lib.GruCellGradJob(None, None, None, 0, ptr(fwd["gates"]), hp, ldh, ptr(drh, 1), 2 * D + 1, rep, ptr(dP), None, ptr(darz), ptr(part))
    assert lib.gnnmp_gru_cell_grad_f32(0, ctypes.byref(job), N, T, t, D, stream) == A.OK, lib.gnnmp_last_error()
    return dict(dP=dP, dac=dac, darz=darz, part=part, part1=part1, keep=(dy, carry, c2, drh))


@gpu
@pytest.mark.parametrize("hkind", RR.H_KINDS)
@pytest.mark.parametrize("t", RR.GATE_TS)
@pytest.mark.parametrize("N", RR.GATE_NS)
@pytest.mark.parametrize("D", RR.GATE_DS)
def test_gru_cell_forward_and_pullback_against_float64(lib, D, N, t, hkind):
    """both phases forward and back within 1e-5 of float64; the state as [N][D] with a stride, as one vector, as NULL; hout strided into a
    NaN panel whose other columns stay NaN, written once (GConvGRU) and twice (DCGRU); only step t of gates / y / dP written; the carry
    as none, one and two addends; two runs give equal bits"""
    import torch
    T = RR.GATE_T
    ops = RR.gate_case("gru", N, D)
    for rep, carries in ((1, (True, True)), (2, (True, True)), (1, (False, False)), (2, (False, True))):
        fwd = _gru_run(lib, ops, hkind, t, rep, N, D, with_hout1=rep == 1 or t == 0)
        bwd = _gru_grad_run(lib, ops, fwd, hkind, t, rep, carries, N, D)
        torch.cuda.synchronize()
        ref = RR.gru_backward(ops, hkind, t, rep, carries)
        g = fwd["gates"][:, t]
        close(g[:, :D], ref["r"], "r"), close(g[:, D:2 * D], ref["z"], "z"), close(g[:, 2 * D:], ref["c"], "c")
        close(fwd["y"][:, t], ref["hn"], "h'")
        others = [k for k in range(T) if k != t]
        assert bool(torch.isnan(fwd["gates"][:, others]).all()) and bool(torch.isnan(fwd["y"][:, others]).all())
        for j in range(rep):
            if hkind == "null":
                assert not bool(fwd["rh"][:, 2 + j * D:2 + (j + 1) * D].any())
            else:
                close(fwd["rh"][:, 2 + j * D:2 + (j + 1) * D], ref["rh"], "r h")
            if rep == 1 or t == 0:
                close(fwd["hn"][:, 2 + j * D:2 + (j + 1) * D], ref["hn"], "hout of phase 1")
        for pan in (fwd["rh"], fwd["hn"]):
            assert bool(torch.isnan(pan[:, :2]).all()) and bool(torch.isnan(pan[:, 2 + rep * D:]).all())
        if not (rep == 1 or t == 0):
            assert bool(torch.isnan(fwd["hn"]).all()), "phase 1 with a NULL hout wrote one"
        d = bwd["dP"][:, t]
        if hkind == "null":                                  # h = 0: dr_pre is an exact zero
            assert not bool(d[:, :D].any()) and not bool(bwd["darz"][:, :D].any())
        else:
            close(d[:, :D], ref["dr"], "dr_pre"), close(bwd["darz"][:, :D], ref["dr"], "darz r")
        close(d[:, D:2 * D], ref["dz"], "dz_pre"), close(d[:, 2 * D:], ref["dc"], "dc_pre")
        close(bwd["dac"], ref["dc"], "dac"), close(bwd["darz"][:, D:], ref["dz"], "darz z")
        close(bwd["part1"], ref["part1"], "part after phase 1"), close(bwd["part"], ref["part"], "part")
        assert bool(torch.isnan(bwd["dP"][:, others]).all())
        fwd2 = _gru_run(lib, ops, hkind, t, rep, N, D, with_hout1=rep == 1 or t == 0)
        bwd2 = _gru_grad_run(lib, ops, fwd2, hkind, t, rep, carries, N, D)
        torch.cuda.synchronize()
        for k in ("gates", "y", "rh", "hn"):
            assert np.array_equal(tbits(fwd[k]), tbits(fwd2[k])), k
        for k in ("dP", "dac", "darz", "part"):
            assert np.array_equal(tbits(bwd[k]), tbits(bwd2[k])), k


def _lstm_run(lib, ops, ckind, t, N, D, stream=None, with_hout=True):
    from gnnmp import _lib
    T = RR.GATE_T
    c, ldc, coff = _state_dev(ops, ckind)
    P, a, w = dev(ops["P"]), dev(ops["a"]), dev(ops["w"])
    gates, cnew, y = nan(N, T, 4 * D), nan(N, T, D), nan(N, T, D)
    ldo = D + 5
    hout = nan(N, ldo)
    job = _lib.LstmCellJob(ptr(P), ptr(a), ptr(w), ptr(c, coff), ldc, ptr(gates), ptr(cnew), ptr(hout, 2) if with_hout else None, ldo, ptr(y))
    assert lib.gnnmp_lstm_cell_f32(ctypes.byref(job), N, T, t, D, stream) == A.OK, lib.gnnmp_last_error()
    return dict(gates=gates, cnew=cnew, y=y, hout=hout, keep=(P, a, w, c), cptr=(ptr(c, coff), ldc))


def _lstm_grad_run(lib, ops, fwd, t, carries, with_peep, N, D, stream=None):
    from gnnmp import _lib
    T = RR.GATE_T
    dy = dev(ops["dy"])
    ch = nan(N, D + 3)
    ch[:, 1:1 + D] = dev(ops["carry"])
    cc = dev(ops["carry_c"]) if carries[1] else None
    dP, da, dc = nan(N, T, 4 * D), nan(N, 4 * D), nan(N, D)
    peep = nan(N, T, 4 * D) if with_peep else None
    cp, ldc = fwd["cptr"]
    job = _lib.LstmCellGradJob(ptr(dy), ptr(ch, 1) if carries[0] else None, D + 3, ptr(cc), ptr(fwd["gates"]), ptr(fwd["keep"][2]), cp, ldc,
                               ptr(fwd["cnew"]), ptr(dP), ptr(da), ptr(dc), ptr(peep))
    assert lib.gnnmp_lstm_cell_grad_f32(ctypes.byref(job), N, T, t, D, stream) == A.OK, lib.gnnmp_last_error()
    return dict(dP=dP, da=da, dc=dc, peep=peep, keep=(dy, ch, cc))


@gpu
@pytest.mark.parametrize("ckind", RR.H_KINDS)
@pytest.mark.parametrize("t", RR.GATE_TS)
@pytest.mark.parametrize("N", RR.GATE_NS)
@pytest.mark.parametrize("D", RR.GATE_DS)
def test_lstm_cell_forward_and_pullback_against_float64(lib, D, N, t, ckind):
    import torch
    T = RR.GATE_T
    ops = RR.gate_case("lstm", N, D)
    others = [k for k in range(T) if k != t]
    for carries, opt in (((True, True), True), ((False, False), False), ((True, False), True)):
        fwd = _lstm_run(lib, ops, ckind, t, N, D, with_hout=opt)
        bwd = _lstm_grad_run(lib, ops, fwd, t, carries, opt, N, D)
        torch.cuda.synchronize()
        ref = RR.lstm_backward(ops, ckind, t, carries)
        g = fwd["gates"][:, t]
        for q, nm in enumerate("ifgo"):
            close(g[:, q * D:(q + 1) * D], ref[nm], nm)
        close(fwd["cnew"][:, t], ref["cn"], "c'"), close(fwd["y"][:, t], ref["hn"], "h'")
        for k in ("gates", "cnew", "y"):
            assert bool(torch.isnan(fwd[k][:, others]).all()), k
        if opt:
            close(fwd["hout"][:, 2:2 + D], ref["hn"], "hout")
            assert bool(torch.isnan(fwd["hout"][:, :2]).all()) and bool(torch.isnan(fwd["hout"][:, 2 + D:]).all())
        else:
            assert bool(torch.isnan(fwd["hout"]).all())
        close(bwd["da"], ref["da"], "da"), close(bwd["dP"][:, t], ref["da"], "dP[t]"), close(bwd["dc"], ref["dc"], "dc")
        assert bool(torch.isnan(bwd["dP"][:, others]).all())
        if opt:
            if ckind == "null":                              # c = 0: the first three products are exact zeros
                assert not bool(bwd["peep"][:, t, :3 * D].any())
                close(bwd["peep"][:, t, 3 * D:], ref["peep"][:, 3 * D:], "peephole product o")
            else:
                close(bwd["peep"][:, t], ref["peep"], "peephole products")
            assert bool(torch.isnan(bwd["peep"][:, others]).all())
        fwd2 = _lstm_run(lib, ops, ckind, t, N, D, with_hout=opt)
        bwd2 = _lstm_grad_run(lib, ops, fwd2, t, carries, opt, N, D)
        torch.cuda.synchronize()
        for k in ("gates", "cnew", "y", "hout"):
            assert np.array_equal(tbits(fwd[k]), tbits(fwd2[k])), k
        for k in ("dP", "da", "dc"):
            assert np.array_equal(tbits(bwd[k]), tbits(bwd2[k])), k


@gpu
@pytest.mark.parametrize("cell", ["gru", "lstm"])
def test_the_gate_kernels_record_into_a_hip_graph_without_an_eager_call(lib, cell):
    """forward and pullback of a cell captured (thread_local error mode: no allocation, no host wait) and replayed: the eager bits"""
    import torch
    N, D, t = 37, 5, 2
    ops = RR.gate_case(cell, N, D)
    stream = torch.cuda.Stream()
    sp = ctypes.c_void_p(stream.cuda_stream)

    def eager(spv):
        if cell == "gru":
            f = _gru_run(lib, ops, "mat", t, 2, N, D, spv)
            return f, _gru_grad_run(lib, ops, f, "mat", t, 2, (True, True), N, D, spv)
        f = _lstm_run(lib, ops, "mat", t, N, D, spv)
        return f, _lstm_grad_run(lib, ops, f, t, (True, True), True, N, D, spv)
    with torch.cuda.stream(stream):
        f0, b0 = eager(sp)
    torch.cuda.synchronize()
    want = {k: v.clone() for k, v in {**f0, **b0}.items() if isinstance(v, torch.Tensor)}
    from gnnmp import _lib
    T = RR.GATE_T
    outs = [v for k, v in {**f0, **b0}.items() if isinstance(v, torch.Tensor) and k != "part1"]
    for v in outs:
        v.fill_(float("nan"))
    if cell == "gru":
        f0["rh"].fill_(float("nan")), f0["hn"].fill_(float("nan"))
    P, a0, a1, h = f0["keep"][0], f0["keep"][1], f0["keep"][2], f0["keep"][3]
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        g.capture_begin(capture_error_mode="thread_local")
        try:
            if cell == "gru":
                ldh, ldo = 2 * D + 3, 2 * D + 5
                dy, carry, c2, drh = b0["keep"]
                j = _lib.GruCellJob(ptr(P), ptr(a0), ptr(h, 3), ldh, ptr(f0["gates"]), ptr(f0["rh"], 2), ldo, 2, None)
                rcs = [lib.gnnmp_gru_cell_f32(0, ctypes.byref(j), N, T, t, D, sp)]
                j = _lib.GruCellJob(ptr(P), ptr(a1), ptr(h, 3), ldh, ptr(f0["gates"]), ptr(f0["hn"], 2), ldo, 2, ptr(f0["y"]))
                rcs.append(lib.gnnmp_gru_cell_f32(1, ctypes.byref(j), N, T, t, D, sp))
                j = _lib.GruCellGradJob(ptr(dy), ptr(carry), ptr(c2, 1), 2 * D + 1, ptr(f0["gates"]), ptr(h, 3), ldh, None, 2 * D + 1, 2,
                                        ptr(b0["dP"]), ptr(b0["dac"]), ptr(b0["darz"]), ptr(b0["part"]))
                rcs.append(lib.gnnmp_gru_cell_grad_f32(1, ctypes.byref(j), N, T, t, D, sp))
                j = _lib.GruCellGradJob(None, None, None, 0, ptr(f0["gates"]), ptr(h, 3), ldh, ptr(drh, 1), 2 * D + 1, 2, ptr(b0["dP"]), None,
                                        ptr(b0["darz"]), ptr(b0["part"]))
                rcs.append(lib.gnnmp_gru_cell_grad_f32(0, ctypes.byref(j), N, T, t, D, sp))
            else:
                w, c = f0["keep"][2], f0["keep"][3]
                dy, ch, cc = b0["keep"]
                j = _lib.LstmCellJob(ptr(P), ptr(a0), ptr(w), ptr(c, 3), 2 * D + 3, ptr(f0["gates"]), ptr(f0["cnew"]), ptr(f0["hout"], 2), D + 5,
                                     ptr(f0["y"]))
                rcs = [lib.gnnmp_lstm_cell_f32(ctypes.byref(j), N, T, t, D, sp)]
                j = _lib.LstmCellGradJob(ptr(dy), ptr(ch, 1), D + 3, ptr(cc), ptr(f0["gates"]), ptr(w), ptr(c, 3), 2 * D + 3, ptr(f0["cnew"]),
                                         ptr(b0["dP"]), ptr(b0["da"]), ptr(b0["dc"]), ptr(b0["peep"]))
                rcs.append(lib.gnnmp_lstm_cell_grad_f32(ctypes.byref(j), N, T, t, D, sp))
        finally:
            g.capture_end()
    torch.cuda.synchronize()
    assert all(rc == A.OK for rc in rcs), lib.gnnmp_last_error()
    assert bool(torch.isnan(f0["y"]).all()), "work ran while the calls were being recorded"
    g.replay()
    torch.cuda.synchronize()
    for k, v in {**f0, **b0}.items():
        if isinstance(v, torch.Tensor) and k != "part1":
            assert np.array_equal(tbits(v), tbits(want[k])), k
    del g


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU 3: the layers
# ------------------------------------------------------------------------------------------------------------------------------------
MAKE = {"gconv_gru": "GConvGRU", "gconv_lstm": "GConvLSTM", "dcgru": "DCGRU"}
AD = {"gconv_gru": "gconv_gru_ad", "gconv_lstm": "gconv_lstm_ad", "dcgru": "dcgru_ad"}


def make_graph(gname):
    import gnnmp
    s, t, n, w, sizes = RR.graph_of(gname)
    if sizes is None:
        return gnnmp.GNNGraph(dev(s), dev(t), None if w is None else dev(w), num_nodes=n, index_base=0)
    parts, off = [], 0
    for m in sizes:                                          # a batch built by the package from its members
        sel = (s >= off) & (s < off + m)
        parts.append(gnnmp.GNNGraph(dev(s[sel] - off), dev(t[sel] - off), None if w is None else dev(w[sel]), num_nodes=m, index_base=0))
        off += m
    g = gnnmp.batch(parts)
    assert g.num_graphs == len(sizes) and g.num_nodes == n
    return g


def make_layer(c, case):
    """the layer of a case with the case's parameters copied in, every one a leaf that requires a gradient"""
    import gnnmp
    import torch
    kind, _, k, _, bias, _, out = c
    layer = getattr(gnnmp, MAKE[kind])((RR.IN, out), k, bias=bias, seed=1)
    params = layer.cell.parameters()
    assert len(params) == len(case["params"])
    with torch.no_grad():
        for p, v in zip(params, case["params"]):
            assert (p is None) == (v is None)
            if p is not None:
                assert tuple(p.shape) == v.shape
                p.copy_(dev(v))
    for p in params:
        if p is not None:
            p.requires_grad_()
    return layer


def _state_arg(kind, st):
    if kind == "gconv_lstm":
        return None if st[0] is None else (st[0], st[1])
    return st[0]


@gpu
@pytest.mark.parametrize("c", RR.LAYER_CASES, ids=RR.case_id)
def test_layer_forward_and_every_gradient_against_float64(c):
    """forward, Δx, Δstate(s) and the gradient of every parameter (the peepholes included) within 1e-5 of the float64 model, norm-wise
    and element-wise, λmax as the device path took it; layer(g, x) and *_ad have equal bits, and so do two runs; the layer over T steps
    agrees at 1e-5 with the cell stepped T times"""
    import gnnmp
    import torch
    from gnnmp.layers_more import scaled_laplacian_op
    kind, gname, k, T, bias, state, out = c
    case = RR.layer_case(c)
    g = make_graph(gname)
    layer = make_layer(c, case)
    lam = None if kind == "dcgru" else scaled_laplacian_op(g)[3]      # a constant of the graph: the model takes the device's value
    ref = RR.layer_ref(c, lam)
    x = dev(case["x"]).requires_grad_()
    st = [None if a is None else dev(a).requires_grad_() for a in case["state"]]
    params = [p for p in layer.cell.parameters() if p is not None]
    ad = getattr(gnnmp, AD[kind])

    def run():
        y = ad(layer, g, x, _state_arg(kind, st))
        wrt = [x] + [a for a in st if a is not None] + params
        return y.detach(), list(torch.autograd.grad(y, wrt, dev(case["dy"])))
    y, gr = run()
    close(y, ref["y"], "y")
    got = list(gr)
    close(got.pop(0), ref["dx"], "dx")
    for q, r in enumerate(ref["dstate"]):
        if r is not None:
            close(got.pop(0), r, f"dstate {q}")
    for q, r in enumerate(ref["dparams"]):
        if r is not None:
            close(got.pop(0), r, f"dparam {q}")
    assert not got
    with torch.no_grad():
        plain = layer(g, x.detach(), _state_arg(kind, [None if a is None else a.detach() for a in st]))
    assert np.array_equal(tbits(plain), tbits(y)), "layer(g, x) and the *_ad forward differ"
    y2, gr2 = run()
    assert np.array_equal(tbits(y2), tbits(y)) and all(np.array_equal(tbits(a), tbits(b)) for a, b in zip(gr, gr2))
    with torch.no_grad():
        s_ = _state_arg(kind, [None if a is None else a.detach() for a in st])
        ys = []
        for q in range(T):
            yq, s_ = layer.cell(g, x.detach()[:, q].contiguous(), s_)
            ys.append(yq)
    close(torch.stack(ys, 1), ref["y"], "the cell stepped T times")
    close(torch.stack(ys, 1), y.cpu().numpy(), "the cell stepped T times against the layer")


@gpu
def test_pruned_gradients_and_refusals():
    """what needs_input_grad rules out is not computed (None comes back, the rest keeps its bits); float64, a bipartite pair and a wrong
    rank or width are refused by name"""
    import gnnmp
    import torch
    c = next(q for q in RR.LAYER_CASES if q[0] == "gconv_lstm" and q[2] == 3 and q[3] == 4 and q[5] == "mat")
    case = RR.layer_case(c)
    g = make_graph(c[1])
    layer = make_layer(c, case)
    params = [p for p in layer.cell.parameters() if p is not None]
    x = dev(case["x"]).requires_grad_()
    h, cc = (dev(a).requires_grad_() for a in case["state"])
    dy = dev(case["dy"])
    full = torch.autograd.grad(gnnmp.gconv_lstm_ad(layer, g, x, (h, cc)), [x, h, cc] + params, dy)
    only_x = torch.autograd.grad(gnnmp.gconv_lstm_ad(layer, g, x, (h.detach(), cc.detach())), [x], dy)
    assert np.array_equal(tbits(only_x[0]), tbits(full[0]))
    for p in params:
        p.requires_grad_(False)
    y = gnnmp.gconv_lstm_ad(layer, g, x.detach(), (h, cc.detach()))
    only_h = torch.autograd.grad(y, [h], dy)
    assert np.array_equal(tbits(only_h[0]), tbits(full[1]))
    for fn, make in ((gnnmp.gconv_gru_ad, gnnmp.GConvGRU), (gnnmp.gconv_lstm_ad, gnnmp.GConvLSTM), (gnnmp.dcgru_ad, gnnmp.DCGRU)):
        lay = make((RR.IN, 4), 2, seed=0)
        xs = x.detach()
        with pytest.raises(ValueError, match=fn.__name__ + ".*Float32"):
            fn(lay, g, xs.double())
        with pytest.raises(NotImplementedError, match=fn.__name__ + ".*bipartite"):
            fn(lay, g, (xs, xs))
        with pytest.raises(ValueError, match=fn.__name__ + r".*\[N\]\[T\]\[5\]"):
            fn(lay, g, xs[:, 0])
        with pytest.raises(ValueError, match=fn.__name__ + r".*\[N\]\[T\]\[5\]"):
            fn(lay, g, xs[:, :, :3])
    with pytest.raises(TypeError, match="gconv_gru_ad: expected a GConvGRUCell"):
        gnnmp.gconv_gru_ad(layer, g, x.detach())


class _Counting:
    """a proxy around the loaded library that counts the gnnmp_* compute calls by name"""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("gnnmp_") or name in ("gnnmp_last_error", "gnnmp_tune_get", "gnnmp_dense_grad_workspace"):
            return fn

        def counted(*a):
            self.calls.append(name)
            return fn(*a)
        return counted


@gpu
@pytest.mark.parametrize("kind,k,budget", [("gconv_gru", 3, 8), ("gconv_lstm", 3, 4), ("dcgru", 2, 12), ("dcgru", 1, 4), ("gconv_gru", 1, 4),
                                           ("dcgru", 3, 16)])
def test_the_forward_keeps_its_launch_budget(monkeypatch, kind, k, budget):
    """n(T) = the gnnmp_* calls of one forward over T steps: n(5) - n(2) is at most three times the per-step budget (GConvGRU 2K + 2,
    GConvLSTM K + 1, DCGRU 4k + 4, 4 for k = 1) — it is exactly that — and the x side's share does not grow with T"""
    import gnnmp
    import torch
    from gnnmp import _lib
    gname = "di_w" if kind == "dcgru" else "bi"
    g = make_graph(gname)
    layer = getattr(gnnmp, MAKE[kind])((RR.IN, RR.OUT), k, seed=2)
    n = g.num_nodes
    layer(g, torch.zeros((n, 1, RR.IN), device="cuda"))       # the graph's caches (λmax, degrees, slot factors) are made once
    proxy = _Counting(_lib.load())
    monkeypatch.setattr(_lib, "_lib", proxy)
    counts = {}
    for T in (2, 5):
        proxy.calls.clear()
        layer(g, torch.zeros((n, T, RR.IN), device="cuda"))
        counts[T] = list(proxy.calls)
    monkeypatch.undo()
    step = len(counts[5]) - len(counts[2])
    print(f"{kind} k = {k}: n(2) = {len(counts[2])}, n(5) = {len(counts[5])}, per step {step / 3}")
    assert step <= 3 * budget and step == 3 * budget
    assert len(counts[2]) - 2 * budget == len(counts[5]) - 5 * budget, "the x side's share grows with T"
    per = [nm for nm in counts[5] if nm in ("gnnmp_gru_cell_f32", "gnnmp_lstm_cell_f32")]
    assert len(per) == (5 if kind == "gconv_lstm" else 10)


@gpu
def test_training_learns_a_diffusion_signal():
    """GNNChain-like GConvGRU(1 => 16, K = 2) -> Dense(16 => 1) learns the one-hop mean of a seeded random signal over a road-like graph
    for each of 4 steps (the task of tests/test_tgcn.py).  Adam (lr 0.01), 60 full-batch steps, fixed seeds.  Bar: the loss ends below
    70 % of where it began (test_tgcn's bar); a model that does not learn stays near 100 %, and the float64 model of
    tests/recurrent_ref.py trained the same way from the same initial weights ends at 2 % (0.347 -> 0.0064)."""
    import gnnmp
    import torch
    from gnnmp.backward import dense_ad
    from test_tgcn import road_graph
    torch.manual_seed(0)
    n, T = 207, 4
    s1, t1 = road_graph(n, seed=21)
    g = gnnmp.GNNGraph(torch.from_numpy(s1).cuda(), torch.from_numpy(t1).cuda(), num_nodes=n)
    st, tt = torch.from_numpy(s1 - 1), torch.from_numpy(t1 - 1)
    deg = torch.zeros(n).index_add(0, tt, torch.ones(len(tt)))
    gen = torch.Generator().manual_seed(1)
    x = torch.randn((n, T, 1), generator=gen)
    target = torch.zeros_like(x)
    for k in range(T):
        target[:, k] = torch.zeros((n, 1)).index_add(0, tt, x[st, k]) / deg[:, None]
    x, target = x.cuda(), target.cuda()
    rnn, head = gnnmp.GConvGRU((1, 16), 2, seed=7), gnnmp.Dense((16, 1), seed=8)
    params = [p.requires_grad_() for p in rnn.cell.parameters() + [head.weight, head.bias]]
    opt = torch.optim.Adam(params, lr=0.01)
    losses = []
    for _ in range(60):
        loss = ((dense_ad(head, gnnmp.gconv_gru_ad(rnn, g, x)) - target) ** 2).mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(loss.item())
    print(f"loss {losses[0]:.4f} -> {losses[-1]:.4f}")
    assert np.isfinite(losses).all() and losses[-1] < 0.7 * losses[0]


@gpu
@pytest.mark.parametrize("kind", ["gconv_gru", "gconv_lstm", "dcgru"])
def test_a_training_step_replays_with_the_eager_bits(kind):
    """one forward + backward of each layer captured into a HIP graph after an eager warm-up and replayed on new values: the bits of the
    eager step on those values"""
    import gnnmp
    import torch
    c = next(q for q in RR.LAYER_CASES if q[0] == kind and q[2] == 3 and q[3] == 4 and q[6] == RR.OUT)
    case = RR.layer_case(c)
    g = make_graph(c[1])
    layer = make_layer(c, case)
    params = [p for p in layer.cell.parameters() if p is not None]
    x, dy = dev(case["x"]).requires_grad_(), dev(case["dy"])
    st = [None if a is None else dev(a).requires_grad_() for a in case["state"]]
    ad = getattr(gnnmp, AD[kind])

    def step():
        y = ad(layer, g, x, _state_arg(kind, st))
        return (y.detach(),) + tuple(torch.autograd.grad(y, [x] + [a for a in st if a is not None] + params, dy))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.synchronize()
    graph_ = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph_, stream=side):
        outs = step()
    torch.cuda.synchronize()
    rng = np.random.default_rng(77)
    with torch.no_grad():
        x.copy_(dev(rng.standard_normal(case["x"].shape).astype(f32)))
        dy.copy_(dev(rng.standard_normal(case["dy"].shape).astype(f32)))
    graph_.replay()
    torch.cuda.synchronize()
    got = [o.clone() for o in outs]
    with torch.cuda.stream(side):
        eager = step()
    torch.cuda.synchronize()
    for k, (a, b) in enumerate(zip(got, eager)):
        assert np.array_equal(tbits(a), tbits(b)), f"output {k} of the replay differs from the eager step"
    del graph_
