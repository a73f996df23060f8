"""The cases of the tiled attention readouts (csrc/readout_tiled.hip) for the ABI's memory contract and capture checks, beside
tests/abi_cases.py as tests/topk_cases.py is: importing this module registers both exports in TABLE (they only launch);
tests/test_readout_tiled.py runs the checks over them.  The float64 formulas are those of tests/readout_ref.py."""
import numpy as np

import abi_cases as A
import readout_ref as R

FWD, GRAD = "gnnmp_segment_attn_pool_tiled_f32", "gnnmp_segment_attn_pool_tiled_grad_f32"
f32, f64 = np.float32, np.float64


def segs():
    """a boundary on a tile edge, an empty segment in the middle and one at the end, a segment over three tiles, short pieces in one tile"""
    from gnnmp import _lib
    T = _lib.READOUT_TILE_ROWS
    return (1, T - 1, 0, T, T + 1, 2 * T + 3, 1, 2, 3, 0)


def _shapes():
    """(k, D, mode, tags): QUERY (0), one gate weight (1), a gate per channel (2); 16-byte lanes in one feature tile and in two"""
    for k, (D, mode) in enumerate((D, mode) for D in (8, 260) for mode in (0, 1, 2)):
        yield k, D, mode, {"align", "side"} if k == 0 else {"align"} if k == 5 else set()


def _operands(name, D, mode):
    from gnnmp import _lib
    r = A.rng_of(name, D, mode)
    ptr = R.ptr_of(segs())
    N, G, Dg = int(ptr[-1]), len(ptr) - 1, (0, 1, D)[mode]
    x, q = A.F(r, N, D), (A.F(r, G, D) * (2.0 / np.sqrt(D))).astype(f32)            # logits of order one
    gate = (2.0 * A.F(r, N, max(Dg, 1))).astype(f32)
    ws = A.Arr("workspace", "scratch", shape=(_lib.load().gnnmp_segment_attn_tiled_workspace(N, G, D, Dg),))
    return ptr, N, G, Dg, x, q if mode == 0 else None, gate if mode else None, A.F(r, G, D), A.F(r, N, D), ws


def build_forward(ctx):
    for _, D, mode, tags in _shapes():
        ptr, N, G, Dg, x, q, gate, _, _, ws = _operands("segment_attn_pool_tiled", D, mode)
        job = A.Rec("gnnmp_segment_attn_tiled_t", x=A.Arr("x", "in", x), seg_ptr=A.Arr("seg_ptr", "in", ptr),
                    q=A.Arr("q", "in", q) if q is not None else None, gate=A.Arr("gate", "in", gate) if gate is not None else None,
                    r=A.Arr("r", "out", shape=(G, D)), stats=A.Arr("stats", "out", shape=(G, max(Dg, 1), 2)), workspace=ws)
        yield A.mk(FWD, f"D{D}_Dg{Dg}", tags, [job, N, G, D, Dg, A.STREAM],
                   lambda host, a=(x, ptr, q, gate): dict(zip(("r", "stats"), R.pool(a[0].astype(f64), a[1], *R.cast(f64, a[2], a[3])))), no_warmup=True)


def build_grad(ctx):
    for k, D, mode, tags in _shapes():
        ptr, N, G, Dg, x, q, gate, dr, base, ws = _operands("segment_attn_pool_tiled_grad", D, mode)
        x64, q64, g64, dr64, b64 = R.cast(f64, x, q, gate, dr, base)
        r64, st64 = R.pool(x64, ptr, q64, g64)
        how = ("base", "base_is_dx", "none", "no_dx", "only_dx")[k % 5]                     # each output is optional, base MAY BE dx
        want = dict(zip(("dq", "dx", "dgate"), R.pool_grad(dr64, x64, ptr, r64, st64, q64, g64, b64 if how in ("base", "base_is_dx") else None)))
        f = dict(dr=A.Arr("dr", "in", dr), x=A.Arr("x", "in", x), seg_ptr=A.Arr("seg_ptr", "in", ptr), q=A.Arr("q", "in", q) if q is not None else None,
                 gate=A.Arr("gate", "in", gate) if gate is not None else None, r=A.Arr("r", "in", r64.astype(f32)),
                 stats=A.Arr("stats", "in", st64.astype(f32)), base=A.Arr("base", "in", base) if how == "base" else None,
                 dq=A.Arr("dq", "out", shape=(G, D)) if mode == 0 and how != "only_dx" else None,
                 dx=A.Arr("dx", "out", shape=(N, D)) if how != "no_dx" else None,
                 dgate=A.Arr("dgate", "out", shape=(N, Dg)) if mode and how != "only_dx" else None, workspace=ws)
        names = {"dq": "dq", "dx": "dx", "dgate": "dgate"}
        if how == "base_is_dx":
            both = A.Arr("base_dx", "inout", base)
            f["base"], f["dx"], names["dx"] = A.Arr("base", "in", base=both), A.Arr("dx", "out", base=both), "base_dx"
        yield A.mk(GRAD, f"D{D}_Dg{Dg}_{how}", tags, [A.Rec("gnnmp_segment_attn_tiled_grad_t", **f), N, G, D, Dg, A.STREAM],
                   lambda host, want=want, f=f, names=names: {names[nm]: want[nm] for nm in want if f[nm] is not None}, no_warmup=True)


for _name, _build in ((FWD, build_forward), (GRAD, build_grad)):
    A.TABLE.setdefault(_name, A._of_variant(_build))      # as the registry's last lines wrap every builder it holds
