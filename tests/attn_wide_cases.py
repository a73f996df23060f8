"""The cases of the head-tiled attention exports (csrc/attn_wide.hip) for the ABI's memory contract, capture and row-geometry checks,
beside tests/abi_cases.py as tests/readout_tiled_cases.py is: importing this module registers both exports in TABLE (they only launch);
tests/test_attn_wide.py runs the checks over them.  The float64 reference is abi_cases.attn_ref, floors included.

Graphs: the table's hub graph WITHOUT plan-added self loops (isolated rows first, last and interior; rows at the split threshold, just
above it — more than 64 slots with a remainder — and five times it, which a whole-row walk that skipped split rows would miss;
multi-edges), and a relation of 5 sources and 37 destinations with a separate Q.  (H, C): HC below; modes GAT, GATV2 and DOT."""
import numpy as np

import abi_cases as A

FWD, GRAD = "gnnmp_attn_conv_wide_f32", "gnnmp_attn_conv_wide_grad_f32"
f32, f64 = np.float32, np.float64
# (H, C): (v, lanes a head, heads a tile, tiles) of csrc/headgeom.h's head_tiles at 16-byte aligned pointers
HC = {(5, 64): (4, 16, 4, 2),      # the last tile holds one head
      (3, 100): (4, 25, 2, 2),     # a head is not a power of two
      (9, 30): (2, 15, 4, 3),
      (13, 5): (1, 5, 12, 2),
      (2, 256): (4, 64, 1, 2),     # one head a wave
      (4, 16): (4, 4, 4, 1)}       # fits a wave: what the narrow exports take too
REFUSED = (2, 130)                 # 65 lanes of 2 floats a head
SLOPE = 0.2
WIDE = ("Q", "K", "V", "out", "dout", "dQ", "dK", "dV", "dA")


def bipartite(ctx):
    return A._bipartite(ctx, "wide_bi", 5, 37, 150, 91)


def shapes(ctx):
    """(graph, H, C, mode, separate Q, tags, status): every (H, C) in every mode on the hub graph, (5, 64) on the bipartite relation"""
    k = 0
    for H, C in HC:
        for mode in (0, 1, 2):
            tags = ({"side", "ws"} if k == 0 else set()) | ({"align"} if (H, C, mode) in ((3, 100, 1), (5, 64, 2), (13, 5, 0)) else set())
            yield ctx.hub, H, C, mode, k % 2 == 1, tags, A.OK
            k += 1
    for mode in (0, 1, 2):
        yield bipartite(ctx), 5, 64, mode, True, set(), A.OK
    yield ctx.hub, *REFUSED, 1, True, set(), A.EUNSUPPORTED


def align_status(H, C, base=None):
    """a [.][H*C] array aligned for narrower lanes than the head needs to fit a wave: GNNMP_EUNSUPPORTED, nothing written — (3, 100) at
    a 4-byte aligned pointer (100 lanes a head), as abi_cases.att_align states it for the row"""
    d = dict(base or {})
    if C > 64:
        d.update({n: A.EUNSUPPORTED for n in WIDE})
    return d


def operands(export, g, H, C, mode, sepQ):
    r = A.rng_of(export, g.name, H, C, mode)
    D = H * C
    i = dict(Q=A.F(r, g.n_dst, D), K=A.F(r, g.n_src, D), V=A.F(r, g.n_src, D), a=A.F(r, H, (2 * C, C, C)[mode]), bias=A.F(r, D),
             dout=A.F(r, g.n_dst, D))
    Q, V = i["Q"] if sepQ else i["K"], i["V"] if mode == 2 else i["K"]
    return i, Q, V, float(f32(np.sqrt(f32(C))))


def build_forward(ctx):
    for k, (g, H, C, mode, sepQ, tags, status) in enumerate(shapes(ctx)):
        i, Q, V, scale = operands(FWD, g, H, C, mode, sepQ)
        with_b, act, with_stats = k % 2 == 0, (k // 2) % 2, k % 3 != 1
        ref = None
        if status == A.OK:
            R = A.attn_ref(g, False, mode, Q, i["K"], V, i["a"], SLOPE, scale, H, C, i["bias"] if with_b else None, act)
            ref = lambda host, R=R, with_stats=with_stats: {"out": R["out"], **({"stats": R["stats"]} if with_stats else {})}      # noqa: E731
        job = A.Rec("gnnmp_attn_wide_t", Q=A.Arr("Q", "in", i["Q"]) if sepQ else None, K=A.Arr("K", "in", i["K"]),
                    V=A.Arr("V", "in", i["V"]) if mode == 2 else None, a=A.Arr("a", "in", i["a"]) if mode != 2 else None,
                    bias=A.Arr("bias", "in", i["bias"]) if with_b else None, out=A.Arr("out", "out", shape=(g.n_dst, H * C)),
                    stats=A.Arr("stats", "out", shape=(g.n_dst, H, 2)) if with_stats else None, negative_slope=SLOPE, scale=scale, act=act)
        yield A.mk(FWD, f"{g.name}_m{mode}_H{H}_C{C}_q{int(sepQ)}", tags, [A.Pl(g), mode, job, H, C, A.STREAM], ref, status=status,
                   align_status=align_status(H, C), no_warmup=True)


def grad_want(g, R, mode, sepQ, with_da):
    """the outputs of the pullback from abi_cases.attn_ref: without a separate Q (square plan) dK holds the whole gradient of K"""
    dQ, dK = (R["dWx_dst"], R["dWx_src"]) if mode == 0 else (R["dQ"], R["dK"])
    want = {"dQ": A.E(dQ, scale=R["gscale_t"]),
            "dK": A.E(dK, scale=R["gscale_s"]) if sepQ else A.E(dK + dQ, scale=R["gscale_s"] + R["gscale_t"])}
    if mode == 2:
        want["dV"] = R["dV"]
    elif with_da:
        want["da"] = A.E(R["da"], scale=R["gscale"])
    return want


def build_grad(ctx):
    for k, (g, H, C, mode, sepQ, tags, status) in enumerate(shapes(ctx)):
        i, Q, V, scale = operands(GRAD, g, H, C, mode, sepQ)
        D, with_da = H * C, k % 3 != 1
        ref, stats = None, np.zeros((g.n_dst, H, 2), f32)
        if status == A.OK:
            R = A.attn_ref(g, False, mode, Q, i["K"], V, i["a"], SLOPE, scale, H, C, dout=i["dout"], split_dst=True)
            stats = R["stats"].astype(f32)
            ref = lambda host, w=grad_want(g, R, mode, sepQ, with_da): dict(w)      # noqa: E731
        job = A.Rec("gnnmp_attn_wide_grad_t", Q=A.Arr("Q", "in", i["Q"]) if sepQ else None, K=A.Arr("K", "in", i["K"]),
                    V=A.Arr("V", "in", i["V"]) if mode == 2 else None, a=A.Arr("a", "in", i["a"]) if mode != 2 else None,
                    stats=A.Arr("stats", "in", stats), dout=A.Arr("dout", "in", i["dout"]), line=A.Arr("line", "scratch", shape=(g.n_dst, H, 4)),
                    dQ=A.Arr("dQ", "out", shape=(g.n_dst, D)), dK=A.Arr("dK", "out", shape=(g.n_src, D)),
                    dV=A.Arr("dV", "out", shape=(g.n_src, D)) if mode == 2 else None,
                    dA=A.Arr("dA", "scratch", shape=(g.n_dst + (g.n_src if mode == 0 else 0), D)) if mode != 2 else None,
                    da=A.Arr("da", "out", shape=(H, (2 * C, C)[mode])) if mode != 2 and with_da else None, negative_slope=SLOPE, scale=scale)
        yield A.mk(GRAD, f"{g.name}_m{mode}_H{H}_C{C}_q{int(sepQ)}", tags, [A.Pl(g), A.Pl(g, T=True), mode, job, H, C, A.STREAM], ref,
                   status=status, align_status=align_status(H, C, A.LINE_ALIGN), no_warmup=True)


for _name, _build in ((FWD, build_forward), (GRAD, build_grad)):
    A.TABLE.setdefault(_name, A._of_variant(_build))      # as the registry's last lines wrap every builder it holds
