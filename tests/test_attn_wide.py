"""Attention on feature rows wider than a wave (csrc/attn_wide.hip; include/gnnmp.h states the arithmetic): the two *_wide_* exports on
the cases of tests/attn_wide_cases.py, and gat_conv_ad / gatv2_conv_ad / transformer_conv_ad / gatv2_conv / transformer_conv at
heads = 5, out = 64 — calls that raised before the head-tiled kernels existed.  Bound everywhere: 1e-5 of the float64 reference's
scale, norm-wise and element-wise (abi_cases.compare; `close` below for the layers)."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_cases as A  # noqa: E402
import attn_edge_ref as R  # noqa: E402
import attn_wide_cases as WC  # noqa: E402  (registers the cases in A.TABLE)
import test_attn_edge as TE  # noqa: E402  (the layer builders and the norm-wise measure of the narrow layers' tests)

gpu = pytest.mark.gpu
ALL = (WC.FWD, WC.GRAD)
f32, f64 = np.float32, np.float64
dev = TE.dev


def test_head_tiles_header_and_table(tmp_path):
    """csrc/headgeom.h's head_tiles under plain g++ against the table of tests/attn_wide_cases.py, the two refusals, and the exports in
    header, SYMBOLS and registry as launch-only, cold-capturable record exports"""
    from gnnmp import _lib
    from gnnmp.layers_attn import head_tiles
    exe = str(tmp_path / "headtiles_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(A.ROOT, "graphneuralnetworks.jl_amd", "csrc"),
                           os.path.join(A.ROOT, "tests", "c_harness", "headtiles_check.cpp"), "-o", exe])
    hcs = list(WC.HC) + [WC.REFUSED, (3, 100)]
    vec0 = [4 if C % 4 == 0 else 2 if C % 2 == 0 else 1 for _, C in WC.HC] + [2, 1]            # (3, 100) at a 4-byte aligned pointer
    out = subprocess.run([exe] + [str(v) for (H, C), v0 in zip(hcs, vec0) for v in (H, C, v0)], capture_output=True, text=True, check=True).stdout
    rows = [tuple(int(v) for v in line.split()) for line in out.splitlines()]
    for (H, C), (vec, lph, hpt, tiles), got in zip(WC.HC, WC.HC.values(), rows):
        code = lph if lph & (lph - 1) == 0 else 0x10000 | (6 << 8) | lph
        assert got == (vec, lph, code, hpt, tiles, 1) and head_tiles(H, C) == (vec, lph, hpt, tiles), (H, C, got)
    assert [r[5] for r in rows[-2:]] == [0, 0]
    h = A.parse_header()
    need = A.must_be_covered(h[0], _lib.SYMBOLS, h.records)
    for name, rtype in zip(ALL, ("gnnmp_attn_wide_t", "gnnmp_attn_wide_grad_t")):
        assert name in _lib.SYMBOLS and name in need and name in A.capturable()
        assert not any(A.WAITS_OR_ALLOCATES.search(t) for t in A.header_comments_of(name)), name
        assert [f[0] for f in h.records[rtype]] == [n for n, _ in A.struct_of(rtype)._fields_]
        assert all(c.no_warmup for c in A.TABLE[name](A.Ctx(int(h[1]["GNNMP_MIN_LONG_ROW"]))))


@pytest.fixture(scope="module")
def lib():
    from gnnmp import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def ctx(lib):
    return A.Ctx(A.plan_threshold(lib, A.Ctx(int(A.parse_header()[1]["GNNMP_MIN_LONG_ROW"])).hub.E))


@gpu
@pytest.mark.parametrize("export", ALL)
def test_exports_against_float64_and_the_memory_contract(lib, ctx, export):
    """every case: every owed element within 1e-5 of float64 and nothing else written, equal bits on a second call; the refused shapes
    leave everything untouched; any element-aligned pointer (refused by name where the narrowed lanes no longer hold a head); a side stream"""
    import torch
    plans, failures, refusals = A.Plans(lib), [], 0
    try:
        for case in A.TABLE[export](ctx):
            sets = [("natural alignment", None, None), ("second call", None, None)]
            sets += [("side stream", None, torch.cuda.Stream())] if "side" in case.tags else []
            for tag, nbytes in A.SHIFTS.items() if "align" in case.tags else ():
                sets += [(f"{a.name}+{tag}", {a.name: nbytes}, None) for a in case.arrs if a.dtype == np.float32]
            first = None
            for what, shifts, stream in sets:
                rc, slab, host = A.run_case(lib, case, plans, shifts=shifts, stream=stream)
                if rc != case.status and rc in {case.align_status.get(n) for n in shifts or ()}:
                    refusals += 1
                    problems = slab.check({}, untouched=True)
                else:
                    problems = A.verify(case, rc, slab, host)
                if what == "natural alignment":
                    first = slab.outputs()
                elif what == "second call" and case.status == A.OK:
                    problems += [f"'{k}' differs between two calls" for k, v in slab.outputs().items() if not np.array_equal(v, first[k])]
                failures += [f"{case.export}[{case.sid}] {what}: {p}" for p in problems]
    finally:
        plans.close()
    assert not failures, "\n".join(failures)
    assert refusals > 0                                      # (3, 100) at 4-byte aligned pointers: 100 lanes a head


@gpu
@pytest.mark.parametrize("export", ALL)
def test_capture_replay_new_values_and_back_to_back(lib, ctx, export):
    """recorded with no eager call first, replayed, fed new values, replayed twice back to back: the eager bits each time"""
    import torch
    import test_abi_graph_capture as C
    C._require_working_capture()
    plans = A.Plans(lib)
    try:
        (c0,), (c1,) = (C._capture_cases(A.Ctx(ctx.thr, variant=v), export) for v in (0, 1))
        problems = C._record_and_replay(lib, c0, c1, plans, torch.cuda.Stream())
    finally:
        plans.close()
    assert not problems, f"{export}[{c0.sid}]:\n  " + "\n  ".join(problems)


@gpu
@pytest.mark.parametrize("mode", [0, 1, 2], ids=["gat", "gatv2", "dot"])
def test_a_row_that_fits_a_wave_agrees_with_the_narrow_exports(lib, mode):
    """(4, 16) on the hub graph, separate Q: one tile; every output within the bar of the one-pass exports' (their split rows are chunked)"""
    import torch
    import gnnmp
    from gnnmp import _lib as L
    from gnnmp import backward_attn as BA, backward_attn_wide as BW
    H, C, hub = 4, 16, A.hub_graph(64)
    g = gnnmp.GNNGraph(dev(hub.s), dev(hub.t), num_nodes=hub.n)
    i, _, _, scale = WC.operands("narrow", hub, H, C, mode, True)
    Q, K, dout, a = dev(i["Q"]), dev(i["K"]), dev(i["dout"]), dev(i["a"]) if mode != 2 else None
    V = dev(i["V"]) if mode == 2 else None
    out, stats = BW._wide_forward(g.plan(False), mode, Q, K, V, a, WC.SLOPE, scale, None, 0, H, C)
    wide = (out, stats) + BW._wide_backward(g, False, mode, Q, K, V, a, WC.SLOPE, scale, stats, dout, H, C)
    if mode == 0:
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device="cuda")      # noqa: E731
        o, st, line, dsd, dss, dsrc, ddst, da = new(hub.n, H * C), new(hub.n, H, 2), new(hub.n, H, 4), new(hub.n, H), new(hub.n, H), new(hub.n, H * C), new(hub.n, H * C), new(H, 2 * C)
        plan, plan_t, p, sp = g.plan(False), g.plan_transposed(False), L.ptr, L.stream_ptr()
        L.check(lib.gnnmp_gat_conv_stats_f32(plan.handle, p(K), p(Q), p(a), WC.SLOPE, None, 0, p(o), p(st), H, C, sp))
        L.check(lib.gnnmp_gat_conv_grad_f32(plan.handle, plan_t.handle, p(K), p(Q), p(a), WC.SLOPE, p(st), p(dout), p(line), p(dsd), p(dss),
                                            p(dsrc), p(ddst), p(da), H, C, sp))
        narrow = (o, st, ddst, dsrc, None, da)
    else:
        o, st = BA._attn_forward(g.plan(False), mode, Q, K, V, a, WC.SLOPE, scale, None, 0, H, C)
        narrow = (o, st) + BA._attn_backward(g, False, mode, Q, K, V, a, WC.SLOPE, scale, st, dout, H, C)
    torch.cuda.synchronize()
    ne = hub.indeg() > 0                                     # an empty row's den: 0 here, the narrow kernels leave what the header leaves open
    for name, w, n in zip(("out", "stats", "dQ", "dK", "dV", "da"), wide, narrow):
        assert (w is None) == (n is None), name
        if w is not None:
            w, n = (v.cpu().numpy()[ne] if name == "stats" else v.cpu().numpy() for v in (w, n))
            assert A.compare(w, n.astype(f64), A.E(n)) is None, (name, A.compare(w, n.astype(f64), A.E(n)))


def close(got, ref, what):
    """norm-wise by the narrow layers' measure (tests/test_attn_edge.py: close), and element-wise against the array's scale"""
    TE.close(got, ref, what)
    got = got.detach().cpu().numpy() if hasattr(got, "detach") else got
    if np.linalg.norm(ref) >= 1e-6:
        worst = np.abs(got - ref).max() / np.abs(ref).max()
        assert worst <= 1e-5, f"{what}: element-wise {worst:.3e} of the array's scale"


H_L, C_L = 5, 64                                             # 80 lanes of four floats: two head tiles, the second holds one head


def _graph40(loops):
    import gnnmp
    hub = A.hub_graph(64)
    s, t = hub.s - 1, hub.t - 1
    if loops:
        s, t = np.concatenate([s, np.arange(hub.n)]), np.concatenate([t, np.arange(hub.n)])
    return hub, gnnmp.GNNGraph(dev(hub.s), dev(hub.t), num_nodes=hub.n), s, t


@gpu
@pytest.mark.parametrize("concat", [True, False], ids=["concat", "mean"])
@pytest.mark.parametrize("loops", [True, False], ids=["loops", "noloops"])
def test_gat_conv_ad_wide(oracle, loops, concat):
    import gnnmp
    from gnnmp.backward import gat_conv_ad
    hub, g, _, _ = _graph40(loops)
    rng = np.random.default_rng([3, int(loops), int(concat)])
    x, r = rng.standard_normal((hub.n, 7)).astype(f32), rng.standard_normal((hub.n, C_L * (H_L if concat else 1))).astype(f32)
    l = gnnmp.GATConv((7, C_L), "relu", heads=H_L, concat=concat, add_self_loops=loops, seed=11)
    l.bias = dev((0.1 * rng.standard_normal(l.bias.numel())).astype(f32))
    prm = [l.dense_x_weight, l.a, l.bias]
    W, a, b = (p.cpu().numpy() for p in prm)
    for p in prm:
        p.requires_grad_(True)
    xt = dev(x).requires_grad_(True)
    y = gat_conv_ad(l, g, xt)
    kw = dict(heads=H_L, negative_slope=0.2, add_self_loops_=loops, concat=concat)
    close(y, oracle.gat_conv(hub.s, hub.t, hub.n, x, W, a, b, "relu", **kw).astype(f64), "gat forward")
    (y * dev(r)).sum().backward()
    for name, got, ref in zip(("dx", "dW", "da", "db"), (xt.grad, *(p.grad for p in prm)), oracle.grad_gat_conv(hub.s, hub.t, hub.n, x, W, a, b, "relu", r, **kw)):
        close(got, np.asarray(ref, f64), f"gat {name}")


@gpu
@pytest.mark.parametrize("concat", [True, False], ids=["concat", "mean"])
@pytest.mark.parametrize("loops", [True, False], ids=["loops", "noloops"])
@pytest.mark.parametrize("kind", ["gatv2", "transformer"])
def test_gatv2_and_transformer_wide(kind, loops, concat):
    """layer call and *_ad forward, then every gradient; the transformer with its root weight, and its skip connection where loops are on"""
    from gnnmp.backward_attn import gatv2_conv_ad, transformer_conv_ad
    from gnnmp.layers_attn import gatv2_conv, transformer_conv
    hub, g, s, t = _graph40(loops)
    rng = np.random.default_rng([4, kind == "gatv2", int(loops), int(concat)])
    om = C_L * (H_L if concat else 1)
    cin = om if (kind == "transformer" and loops) else 5
    x, r = rng.standard_normal((hub.n, cin)).astype(f32), rng.standard_normal((hub.n, om)).astype(f32)
    if kind == "gatv2":
        p = R.gatv2_params(rng, cin, TE.EIN, H_L, C_L, concat, "relu", edge=False)
        l, fwd, ad, names = TE.make_gatv2(p, cin), gatv2_conv, gatv2_conv_ad, TE.GAT_GRADS
        y64, g64 = R.gatv2_layer(s, t, hub.n, x, None, p)[0], R.gatv2_grad(s, t, hub.n, x, None, p, r)
    else:
        p = R.transformer_params(rng, cin, TE.EIN, H_L, C_L, concat, True, loops, edge=False)
        l, fwd, ad, names = TE.make_transformer(p, cin), transformer_conv, transformer_conv_ad, TE.TR_GRADS
        y64, g64 = R.transformer_layer(s, t, hub.n, x, None, p)[0], R.transformer_grad(s, t, hub.n, x, None, p, r)
    l.add_self_loops = loops
    close(fwd(l, g, dev(x)), y64, f"{kind} forward")
    xt = dev(x).requires_grad_(True)
    y = ad(l, g, xt)
    close(y, y64, f"{kind} forward (ad)")
    (y * dev(r)).sum().backward()
    close(xt.grad, g64["dx"], f"{kind} dx")
    for name, key in names:
        if getattr(l, name) is not None:
            close(getattr(l, name).grad, g64[key], f"{kind} {key}")


@gpu
def test_the_refusals_that_remain_come_by_name():
    """wide rows with e, wide rows with attention dropout, a head wider than a wave: the mirror knows, and says so before any C call"""
    import torch
    import gnnmp
    from gnnmp.backward import gat_conv_ad
    from gnnmp.backward_attn import gatv2_conv_ad, transformer_conv_ad
    from gnnmp.layers_attn import GATv2Conv, TransformerConv, gatv2_conv, transformer_conv
    hub, g, _, _ = _graph40(False)
    x, e = torch.zeros((hub.n, 5), device="cuda"), torch.zeros((hub.E, 3), device="cuda")
    for l, fns in ((GATv2Conv(((5, 3), C_L), heads=H_L, add_self_loops=False), (gatv2_conv, gatv2_conv_ad)),
                   (TransformerConv(((5, 3), C_L), heads=H_L), (transformer_conv, transformer_conv_ad)),
                   (gnnmp.GATConv(((5, 3), C_L), heads=H_L, add_self_loops=False), (gat_conv_ad,))):
        for fn in fns:
            with pytest.raises(AssertionError, match="must fit one wave"):
                fn(l, g, x, e)
    for l, fns in ((GATv2Conv((5, C_L), heads=H_L, dropout=0.25), (gatv2_conv, gatv2_conv_ad)), (gnnmp.GATConv((5, C_L), heads=H_L, dropout=0.25), (gat_conv_ad,))):
        for fn in fns:
            with pytest.raises(ValueError, match="does not fit one wave"):
                fn(l, g, x)
    for l, fns in ((GATv2Conv((5, 130), heads=2), (gatv2_conv, gatv2_conv_ad)), (TransformerConv((5, 130), heads=2), (transformer_conv, transformer_conv_ad)),
                   (gnnmp.GATConv((5, 130), heads=2), (gat_conv_ad,))):
        for fn in fns:
            with pytest.raises(ValueError, match="a head must fit one wave"):
                fn(l, g, x)
