"""The tiled route of the attention readouts (csrc/readout_tiled.hip; include/gnnmp.h states the arithmetic): the two *_tiled_* exports
and `route="tiled"` of set2set_ad / global_attention_pool_ad, on the segment table of tests/readout_tiled_cases.py.  The float64
formulas are those of tests/readout_ref.py, the bounds and the device helpers those tests/test_readout_ad.py applies to the
whole-segment route (`close`: 1e-5, norm-wise and element-wise; `judge` for the weight gradients)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_cases as A  # noqa: E402
import readout_ref as R  # noqa: E402
import readout_tiled_cases as TC  # noqa: E402  (registers the cases in A.TABLE)
import test_readout_ad as T  # noqa: E402  (the bounds and the device helpers of the whole-segment route's tests)

gpu = pytest.mark.gpu
ALL = (TC.FWD, TC.GRAD)
WSP = "gnnmp_segment_attn_tiled_workspace"
RECORDS = {TC.FWD: ("gnnmp_segment_attn_tiled_t", "SegmentAttnTiledJob"), TC.GRAD: ("gnnmp_segment_attn_tiled_grad_t", "SegmentAttnTiledGradJob")}


def test_header_symbols_library_records_and_route():
    import torch
    from gnnmp import _lib, backward_readout as BR
    h = A.parse_header()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    assert all(name in h[0] and name in _lib.SYMBOLS and name in exported for name in ALL + (WSP,))
    assert int(h[1]["GNNMP_READOUT_TILE_ROWS"]) == _lib.READOUT_TILE_ROWS
    why = {}
    need = A.must_be_covered(h[0], _lib.SYMBOLS, h.records, why)
    for name in ALL:          # launch-only, owed to the case table through their records, and in it
        assert [p[0] for p in h[0][name]] == ["job", "N", "G", "D", "Dg", "stream"] and h[0][name][0][2]
        assert not any(A.WAITS_OR_ALLOCATES.search(t) for t in A.header_comments_of(name)), name
        assert name in need and why[name] == "record" and name in A.capturable()
        rtype, cls = RECORDS[name]
        st = getattr(_lib, cls)
        assert A.struct_of(rtype) is st and [f[0] for f in h.records[rtype]] == [n for n, _ in st._fields_]
        assert ctypes.sizeof(st) == 8 * len(st._fields_) and st._fields_[-1][0] == "workspace"
    ws, Rr = _lib.load().gnnmp_segment_attn_tiled_workspace, _lib.READOUT_TILE_ROWS
    for N, G, D, Dg in ((0, 0, 1, 0), (1, 1, 1, 1), (Rr, 3, 8, 0), (Rr + 1, 3, 8, 8), (32 * 1024, 32, 64, 1), (10 ** 7, 1, 260, 260)):
        assert ws(N, G, D, Dg) == (-(-N // Rr) + G) * (D + 2 * max(Dg, 1)), (N, G, D, Dg)
    assert ws(-1, 1, 8, 0) == 0 and ws(1, -1, 8, 0) == 0 and ws(1, 1, 0, 0) == 0
    assert BR.readout_route(700, 1) == "whole" and BR.readout_route(32 * 1024, 32) == "tiled" and 700 < BR.TILED_MEAN_ROWS <= 1024
    with pytest.raises(ValueError, match="segment_attn_pool: route 'chunks'"):
        BR.segment_attn_pool(torch.zeros(2, 2), torch.zeros(2, dtype=torch.int64), q=torch.zeros(1, 2), route="chunks")


DEFAULTS = dict(dr=1, x=2, seg_ptr=3, q=4, gate=None, r=6, stats=7, base=None, dq=9, dx=10, dgate=None, workspace=12)


def _call(lib, export, job=True, N=7, G=2, D=4, Dg=0, **kw):
    """one call; a field is a device tensor, or a small integer that stands for a pointer that is no memory (the call must refuse first)"""
    from gnnmp import _lib
    st = getattr(_lib, RECORDS[export][1])
    j = st(*[T.ptr(v) if hasattr(v, "data_ptr") else T.P_(v) for v in ({**DEFAULTS, **kw}[f] for f, _ in st._fields_)])
    return getattr(lib, export)(ctypes.byref(j) if job else None, N, G, D, Dg, None)


def test_refusals_come_before_any_launch():
    """the whole-segment pair's refusals under the tiled exports' names, a NULL workspace, and OK without a launch for G = 0 or N = 0"""
    from gnnmp import _lib
    lib = _lib.load()
    err, big, gate = lib.gnnmp_last_error, _lib.READOUT_MAX_D, dict(q=None, gate=5)
    both = [(dict(job=False), b"null job"), (dict(x=None), b"null x"), (dict(seg_ptr=None), b"null seg_ptr"), (dict(r=None), b"null r"),
            (dict(stats=None), b"null stats"), (dict(workspace=None), b"null workspace"), (dict(gate=5), b"exactly one of q and gate"),
            (dict(q=None), b"exactly one of q and gate"), (dict(Dg=1), b"does not go with q"), (dict(Dg=0, **gate), b"does not go with gate"),
            (dict(N=-1), b"negative"), (dict(G=-1), b"negative")]
    both += [(dict(Dg=v), b"bad Dg") for v in (-1, 2, 5, 2 ** 40)] + [(dict(D=v), b"bad D") for v in (0, -1, big + 1)]
    grad = [(dict(dr=None), b"null dr"), (dict(dq=None, dx=None), b"dq and dx are both null"), (dict(dgate=11), b"dgate in query mode"),
            (dict(Dg=1, dq=None, dx=None, **gate), b"dgate and dx are both null"), (dict(Dg=1, dgate=11, **gate), b"dq in gate mode"),
            (dict(base=8, dx=None), b"base without dx")]
    for export, who, table in ((TC.FWD, b"segment_attn_pool_tiled:", both), (TC.GRAD, b"segment_attn_pool_tiled_grad:", both + grad)):
        for bad, word in table:
            assert _call(lib, export, **bad) == _lib.EINVAL and who in err() and word in err(), (export, bad, err())
        for kw in (dict(G=0), dict(N=0), dict(N=0, x=None), dict(N=0, Dg=4, dq=None, **gate)):
            assert _call(lib, export, **kw) == _lib.OK, (export, kw)


def run_pool(lib, D, Dg):
    import torch
    x, sp, q, gate, _, _ = R.pool_case(D, Dg, 0, TC.segs())
    N, G = x.shape[0], len(sp) - 1
    xd, spd, qd, gd = T.dev(x), T.dev(sp), None if q is None else T.dev(q), None if gate is None else T.dev(gate)
    r, stats, ws = T.nan(G, D), T.nan(G, max(Dg, 1), 2), T.nan(lib.gnnmp_segment_attn_tiled_workspace(N, G, D, Dg))
    assert _call(lib, TC.FWD, x=xd, seg_ptr=spd, q=qd, gate=gd, r=r, stats=stats, workspace=ws, N=N, G=G, D=D, Dg=Dg) == A.OK, lib.gnnmp_last_error()
    torch.cuda.synchronize()
    return r.cpu().numpy(), stats.cpu().numpy()


def run_grad(lib, D, Dg, r, stats, base=None, want=("dq", "dx", "dgate"), export=TC.GRAD):
    """(dq, dx, dgate) of the tiled pullback or, export = T.GRAD, of the whole-segment one; base: None | 'separate' | 'alias'"""
    import torch
    x, sp, q, gate, dr, b = R.pool_case(D, Dg, 0, TC.segs())
    N, G = x.shape[0], len(sp) - 1
    dq = T.nan(G, D) if Dg == 0 and "dq" in want else None
    dgate = T.nan(N, Dg) if Dg and "dgate" in want else None
    dx = (T.dev(b) if base == "alias" else T.nan(N, D)) if "dx" in want else None
    ops = dict(dr=T.dev(dr), x=T.dev(x), seg_ptr=T.dev(sp), q=None if q is None else T.dev(q), gate=None if gate is None else T.dev(gate),
               r=T.dev(r), stats=T.dev(stats), base=None if base is None else dx if base == "alias" else T.dev(b), dq=dq, dx=dx, dgate=dgate)
    if export == TC.GRAD:
        ops["workspace"] = T.nan(lib.gnnmp_segment_attn_tiled_workspace(N, G, D, Dg))
        rc = _call(lib, export, N=N, G=G, D=D, Dg=Dg, **ops)
    else:
        rc = T.call_grad(lib, *[T.ptr(v) for v in ops.values()], N, G, D, Dg)
    assert rc == A.OK, lib.gnnmp_last_error()
    torch.cuda.synchronize()
    return tuple(None if v is None else v.cpu().numpy() for v in (dq, dx, dgate))


@pytest.fixture(scope="module")
def lib():
    from gnnmp import _lib
    return _lib.load()


@gpu
@pytest.mark.parametrize("mode", T.MODES)
@pytest.mark.parametrize("D", [8, 6, 5, 260])
def test_tiled_exports_against_float64(lib, D, mode):
    """D = 8, 260: 16-byte lanes (260: a second feature tile), 6: 8-byte, 5: 4-byte.  Pieces shared by 128, 64, 32 and 4 lane groups and
    short pieces dealt to them; the empty segments (2 and 9) give exact zeros"""
    Dg = T.dg_of(mode, D)
    ref = R.pool_ref(D, Dg, 0, "float64", TC.segs())
    k = 0 if mode == "query" else 2
    r, stats = run_pool(lib, D, Dg)
    T.close(r, ref["r"], "r")
    T.close(stats, ref["stats"], "stats")
    empty = [g for g, n in enumerate(TC.segs()) if n == 0]
    assert len(empty) == 2 and not r[empty].any() and not stats[empty].any()
    assert all(np.array_equal(T.bits(a), T.bits(b)) for a, b in zip((r, stats), run_pool(lib, D, Dg)))
    full = run_grad(lib, D, Dg, r, stats)
    whole = run_grad(lib, D, Dg, r, stats, export=T.GRAD)      # the stats layout is interchangeable
    for got in (full, whole):
        T.close(got[1], ref["dx"], "dx")
        T.close(got[k], ref["dq" if mode == "query" else "dgate"], "dq" if mode == "query" else "dgate")
        assert got[2 - k] is None and (mode != "query" or not got[0][empty].any())
    again, only_dx = run_grad(lib, D, Dg, r, stats), run_grad(lib, D, Dg, r, stats, want=("dx",))
    only_other = run_grad(lib, D, Dg, r, stats, want=("dq" if mode == "query" else "dgate",))
    assert np.array_equal(T.bits(again[1]), T.bits(full[1])) and np.array_equal(T.bits(again[k]), T.bits(full[k]))
    assert np.array_equal(T.bits(only_dx[1]), T.bits(full[1])) and only_dx[k] is None
    assert np.array_equal(T.bits(only_other[k]), T.bits(full[k])) and only_other[1] is None
    sep, alias = run_grad(lib, D, Dg, r, stats, base="separate"), run_grad(lib, D, Dg, r, stats, base="alias")
    T.close(sep[1], ref["dx_base"], "dx with base")
    assert np.array_equal(T.bits(sep[1]), T.bits(alias[1])) and np.array_equal(T.bits(sep[k]), T.bits(alias[k]))
    assert np.array_equal(T.bits(sep[k]), T.bits(full[k]))


# the memory contract and the capture, over the cases of tests/readout_tiled_cases.py with the registry's own helpers
@gpu
@pytest.mark.parametrize("export", ALL)
def test_the_memory_contract(lib, export):
    """every owed element written, nothing before or after any array or behind the workspace of the size the library returned"""
    import torch
    plans, failures = A.Plans(lib), []
    for case in A.TABLE[export](A.Ctx(int(A.parse_header()[1]["GNNMP_MIN_LONG_ROW"]))):
        sets = [("natural alignment", None, None)] + ([("side stream", None, torch.cuda.Stream())] if "side" in case.tags else [])
        for tag, nbytes in A.SHIFTS.items() if "align" in case.tags else ():
            sets += [(f"{a.name}+{tag}", {a.name: nbytes}, None) for a in case.arrs if a.dtype == np.float32]
        for what, shifts, stream in sets:
            rc, slab, host = A.run_case(lib, case, plans, shifts=shifts, stream=stream)
            failures += [f"{case.export}[{case.sid}] {what}: {p}" for p in A.verify(case, rc, slab, host)]
    assert not failures, "\n".join(failures)


@gpu
@pytest.mark.parametrize("export", ALL)
def test_capture_replay_new_values_and_back_to_back(lib, export):
    """recorded with no eager call first, replayed, fed new values, replayed twice back to back: the eager bits each time"""
    import torch
    import test_abi_graph_capture as C
    C._require_working_capture()
    (c0,), (c1,) = (C._capture_cases(C._dry_ctx(v), export) for v in (0, 1))      # (the cases take no plan: the dry threshold will do)
    assert c0.no_warmup
    problems = C._record_and_replay(lib, c0, c1, A.Plans(lib), torch.cuda.Stream())
    assert not problems, f"{export}[{c0.sid}]:\n  " + "\n  ".join(problems)


# the layers with route="tiled", by the bounds tests/test_readout_ad.py applies to route "whole"
@gpu
@pytest.mark.parametrize("iters", T.LAYER_ITERS)
def test_set2set_ad_tiled_against_the_reference(iters):
    import torch
    import gnnmp
    n, segs = 8, TC.segs()
    x, sp, Wi, Wh, b, dout = R.set2set_case(n, 0, segs)
    ref, rest = R.set2set_ref(n, iters, 0, "float64", segs), R.set2set_ref(n, iters, 0, "float32", segs)
    l = T.make_set2set(n, iters, Wi, Wh, b)
    xt = T.dev(x).requires_grad_(True)
    y = gnnmp.set2set_ad(l, T.batch_graph(segs), xt, route="tiled")
    (y * T.dev(dout)).sum().backward()
    torch.cuda.synchronize()
    T.close(y.detach().cpu().numpy(), ref["y"], "set2set_ad")
    T.close(xt.grad.cpu().numpy(), ref["dx"], "dx")
    for p, k, m in ((l.Wi, "dWi", "mWi"), (l.Wh, "dWh", "mWh"), (l.b, "db", "mb")):
        T.judge(p.grad.cpu().numpy(), rest[k], ref[k], ref[m], ref["n"], k)


@gpu
@pytest.mark.parametrize("Dg", ["one", "all"])
def test_global_attention_pool_ad_tiled_against_the_reference(Dg):
    import torch
    import gnnmp
    from gnnmp.layers_khop import GlobalAttentionPool
    segs = TC.segs()
    x, sp, fgate, ffeat, dr = R.gap_case(T.GAP_D, Dg, True, segs)
    ref, rest = R.gap_ref(T.GAP_D, Dg, True, "float64", segs), R.gap_ref(T.GAP_D, Dg, True, "float32", segs)
    fg, ff = T.make_chain(fgate), T.make_chain(ffeat)
    xt = T.dev(x).requires_grad_(True)
    y = gnnmp.global_attention_pool_ad(GlobalAttentionPool(fg, ff), T.batch_graph(segs), xt, route="tiled")
    (y * T.dev(dr)).sum().backward()
    torch.cuda.synchronize()
    T.close(y.detach().cpu().numpy(), ref["y"], "global_attention_pool_ad")
    T.close(xt.grad.cpu().numpy(), ref["dx"], "dx")
    for name, chain in (("fgate", fg), ("ffeat", ff)):
        for k, d in enumerate(chain):
            for p, i, what in ((d.weight, 0, "W"), (d.bias, 1, "b")):
                T.judge(p.grad.cpu().numpy(), rest[name][k][i], ref[name][k][i], ref[name][k][i + 2], x.shape[0], f"{name}[{k}].{what}")
