"""Edge features in GATv2Conv and TransformerConv, forward and training (csrc/attn_edge.hip; include/gnnmp.h states the arithmetic;
tests/attn_edge_ref.py is the float64 reference, pinned by tests/test_attn_edge_ref.py).

Without a GPU: the two exports are in header, SYMBOLS and library and take const plans and const host records whose ctypes mirrors have
the header's layout; every refusal comes before any HIP call; the constructors take (in, ein) => out.

On the GPU, on ONE graph of 48 nodes whose edge list is shuffled (plan slot != edge position): a node without in-edges, one with one,
one with nine, a hub of 600 in-edges, a hub of 600 out-edges and twenty (s, t) pairs listed twice with different e — forward and every
gradient of both layers against float64 at the bars of tests/test_attn_layers.py and tests/test_backward_attn.py (1e-5, norm-wise), with
the e-less pullback on the same graph as the control; the memory contract of the raw exports at every alignment; capture without an
eager call; equal bits of two calls; the e-less paths untouched bit for bit; the host's refusals."""
import ctypes
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_cases as A  # noqa: E402
import attn_edge_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FWD, GRAD = "gnnmp_attn_conv_edge_f32", "gnnmp_attn_conv_edge_grad_f32"
gpu = pytest.mark.gpu
f32, f64 = np.float32, np.float64
GAT, GATV2, DOT, COS = 0, 1, 2, 3
MODE_NAME = {GATV2: "gatv2", DOT: "dot"}
WIDTHS = [(1, 8), (3, 4), (2, 6), (2, 7)]      # v = 4, 4, 2, 1; the last head is 7 lanes wide: no power of two
EIN, SLOPE = 3, 0.2
RECORDS = {FWD: ("gnnmp_attn_edge_t", "AttnEdgeJob", ("Q", "K", "V", "F", "a", "bias", "out", "stats", "negative_slope", "scale", "act")),
           GRAD: ("gnnmp_attn_edge_grad_t", "AttnEdgeGradJob", ("Q", "K", "V", "F", "a", "stats", "dout", "line", "dQ", "dK", "dV", "dF", "dA",
                                                                "da", "negative_slope", "scale"))}
PARAMS = {FWD: ["plan", "mode", "job", "H", "C", "stream"], GRAD: ["plan", "plan_t", "mode", "job", "H", "C", "stream"]}


# ------------------------------------------------------------------------------------------------------------------------------------
# CPU: the ABI and the constructors
# ------------------------------------------------------------------------------------------------------------------------------------
def test_header_symbols_and_library_carry_the_exports():
    from gnnmp import _lib
    header = open(os.path.join(ROOT, "include", "gnnmp.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    internal = header.index("GNNMP_INTERNAL")
    for name in (FWD, GRAD):
        assert f"int {name}(" in header and header.index(f"int {name}(") < internal, name
        assert name in _lib.SYMBOLS and name in exported, name
        assert "} " + RECORDS[name][0] + ";" in header
    assert "conv.jl:171-214" in header[:internal] and ":553-629" in header[:internal]
    assert "tests/test_attn_edge.py" in header[:header.index("#ifndef GNNMP_H")]


@pytest.mark.parametrize("export", [FWD, GRAD])
def test_the_exports_take_const_plans_and_const_host_records(export):
    """every pointer travels in the const host record: tests/abi_cases.py owes no case, this file carries the memory-contract and capture
    checks.  The ctypes records have the layout of the header's structs: names, offsets, size."""
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


def _fwd(lib, plan, mode=GATV2, job=True, Q=1, K=2, V=None, F=3, a=4, bias=5, out=6, stats=7, act=0, H=2, C=4):
    from gnnmp import _lib
    j = _lib.AttnEdgeJob(P_(Q), P_(K), P_(V), P_(F), P_(a), P_(bias), P_(out), P_(stats), 0.2, 2.0, act)
    return lib.gnnmp_attn_conv_edge_f32(plan, mode, ctypes.byref(j) if job else None, H, C, None)


def _grad(lib, plan, plan_t, mode=GATV2, job=True, Q=1, K=2, V=None, F=3, a=4, stats=5, dout=6, line=7, dQ=8, dK=9, dV=10, dF=11, dA=12,
          da=13, H=2, C=4):
    from gnnmp import _lib
    j = _lib.AttnEdgeGradJob(P_(Q), P_(K), P_(V), P_(F), P_(a), P_(stats), P_(dout), P_(line), P_(dQ), P_(dK), P_(dV), P_(dF), P_(dA),
                             P_(da), 0.2, 2.0)
    return lib.gnnmp_attn_conv_edge_grad_f32(plan, plan_t, mode, ctypes.byref(j) if job else None, H, C, None)


def test_refusals_come_before_any_hip_call():
    """on a machine without a device, on pointers that are not memory: NULL F, a self-loop plan, mode GAT / COS, a row wider than a wave,
    and the rest of the header's list"""
    from gnnmp import _lib
    lib = _lib.load()
    EINVAL, EUNSUPPORTED, err = _lib.EINVAL, A.EUNSUPPORTED, lib.gnnmp_last_error
    sq, sq_t = _FakePlan(n_src=5, n_dst=5, n_edges=7, n_total=7), _FakePlan(n_src=5, n_dst=5, n_edges=7, n_total=7)
    loops, tall = _FakePlan(n_src=5, n_dst=5, n_edges=7, n_total=12), _FakePlan(n_src=6, n_dst=6, n_edges=7, n_total=7)
    pl, pt, lp, tl = (ctypes.addressof(v) for v in (sq, sq_t, loops, tall))
    for call in (lambda **kw: _fwd(lib, **kw), lambda **kw: _grad(lib, plan_t=pt, **kw)):
        assert call(plan=None) == EINVAL and b"null plan" in err()
        assert call(plan=pl, job=False) == EINVAL and b"null job" in err()
        assert call(plan=pl, F=None) == EINVAL and b"null F" in err()
        assert call(plan=lp) == EINVAL and b"self loops" in err() and b"conv.jl:178-181" in err()
        for mode in (GAT, COS, -1, 4):
            assert call(plan=pl, mode=mode) == EINVAL and b"mode" in err(), mode
        for H, C in ((0, 4), (2, 0), (-1, 4), (1 << 11, 1 << 11)):
            assert call(plan=pl, H=H, C=C) == EINVAL and b"bad H/C" in err(), (H, C)
        for mode in (GATV2, DOT):                         # 65 lanes of 4, 2 and 1 floats: wider than a wave
            for H, C in ((65, 4), (1, 130), (5, 13)):
                assert call(plan=pl, mode=mode, V=(20 if mode == DOT else None), H=H, C=C) == EUNSUPPORTED and b"fit one wave" in err()
        assert call(plan=pl, mode=GATV2, V=20) == EINVAL                      # a separate V needs DOT
        assert call(plan=pl, mode=GATV2, a=None) == EINVAL and b"null pointer" in err()
    assert _fwd(lib, pl, act=2) == EINVAL and b"bad act" in err()
    assert _fwd(lib, pl, out=None) == EINVAL and b"null pointer" in err()
    assert _grad(lib, pl, None) == EINVAL and b"null plan_t" in err()
    assert _grad(lib, pl, tl) == EINVAL and b"not the transpose" in err()
    assert _grad(lib, pl, pt, dF=None) == EINVAL and b"null F / dF" in err()
    for name in ("stats", "dout", "line", "dQ", "dK", "dA"):
        assert _grad(lib, pl, pt, **{name: None}) == EINVAL and b"null pointer" in err(), name
    assert _grad(lib, pl, pt, mode=DOT, V=20, dV=None) == EINVAL and b"null pointer" in err()
    none = _FakePlan(n_src=0, n_dst=0, n_edges=0, n_total=0)
    pn = ctypes.addressof(none)
    assert _fwd(lib, pn, F=None) == _lib.OK and _grad(lib, pn, pn, F=None, dF=None) == _lib.OK       # nothing to do: no launch


def test_constructors_take_edge_channels():
    """GATv2Conv((in, ein) => out) / TransformerConv((in, ein) => out): field names, shapes, parameters(), and the reference's assertion
    on ein with add_self_loops (GraphNeuralNetworks/src/layers/conv.jl:446-448, 1515-1517)"""
    from gnnmp.layers_attn import GATv2Conv, TransformerConv
    msg = "Using edge features and setting add_self_loops=true at the same time is not yet supported."
    l = GATv2Conv(((5, 3), 4), "relu", heads=2, add_self_loops=False, device="cpu", seed=1)
    assert l.ein == 3 and tuple(l.dense_e_weight.shape) == (8, 3) and l.dense_e is l.dense_e_weight and l.channel == (5, 4)
    assert GATv2Conv.PARAMETER_NAMES == ("dense_i_weight", "dense_i_bias", "dense_j_weight", "dense_e_weight", "a", "bias")
    assert [p is not None for p in l.parameters()] == [True] * 6
    l0 = GATv2Conv((5, 4), heads=2, device="cpu", seed=1)
    assert l0.dense_e_weight is None and l0.dense_e is None and l0.ein == 0 and l0.parameters()[3] is None
    assert all(bool((getattr(l, n) == getattr(l0, n)).all()) for n in ("dense_i_weight", "dense_j_weight", "a"))      # same seeds as before
    with pytest.raises(AssertionError, match=re.escape(msg)):
        GATv2Conv(((5, 3), 4), heads=2, device="cpu")                          # add_self_loops defaults to true
    t = TransformerConv(((5, 3), 4), heads=2, device="cpu", seed=1)
    assert t.ein == 3 and tuple(t.W6_weight.shape) == (8, 3) and tuple(t.W6_bias.shape) == (8,) and t.channels == (5, 4)
    assert TransformerConv.PARAMETER_NAMES[-2:] == ("W6_weight", "W6_bias") and len(t.parameters()) == 10
    assert TransformerConv(((5, 3), 4), heads=2, bias_qkv=False, device="cpu").W6_bias is None
    t0 = TransformerConv((5, 4), heads=2, device="cpu", seed=1)
    assert t0.W6_weight is None and t0.W6_bias is None and t0.parameters()[-2:] == [None, None]
    with pytest.raises(AssertionError, match=re.escape(msg)):
        TransformerConv(((5, 3), 4), heads=2, add_self_loops=True, device="cpu")
    for kw in (dict(gating=True), dict(batch_norm=True), dict(ff_channels=8)):
        with pytest.raises(AssertionError):
            TransformerConv(((5, 3), 4), device="cpu", **kw)


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU helpers: the graph, the core cases (raw exports) and the layer cases, each computed once
# ------------------------------------------------------------------------------------------------------------------------------------
def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def ptr(v):
    return None if v is None else ctypes.c_void_p(v.data_ptr())


def close(got, ref, what, tol=1e-5):
    """tests/test_backward_attn.py's measure (norm-wise; a gradient that vanishes identically: |got| <= 1e-3), which is also
    tests/test_attn_layers.py's for the forward.  Returns the ratio"""
    got = got.detach().cpu().numpy() if hasattr(got, "detach") else got
    assert got.shape == ref.shape, what
    assert np.all(np.isfinite(got)), what
    if np.linalg.norm(ref) < 1e-6:
        assert np.linalg.norm(got) <= 1e-3, what
        return 0.0
    ratio = np.linalg.norm(got - ref) / np.linalg.norm(ref)
    print(f"{what}: |got - ref| / |ref| = {ratio:.3e}")
    assert ratio <= tol, f"{what}: {ratio:.3e} > {tol:g}"
    return ratio


@pytest.fixture(scope="module")
def lib():
    import torch
    assert torch.cuda.is_available()
    from gnnmp import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def graph(lib):
    import gnnmp
    s, t = R.graph()
    R.assert_graph(s, t)
    g = gnnmp.GNNGraph(dev(s), dev(t), num_nodes=R.N_NODES, index_base=0)
    plan, plan_t = g.plan(False), g.plan_transposed(False)
    assert R.HUB > plan.long_thresh and plan.n_long >= 1 and plan_t.n_long >= 1      # the plans DO split the hubs
    return g, s, t


@functools.lru_cache(maxsize=None)
def core_case(mode, H, C, seed=0, E=None):
    """float32 operands of one raw call and the float64 results: dict(inp=..., fwd=..., grad=...)"""
    s, t = R.graph()
    if E is not None:
        s, t = s[:E], t[:E]
    n, rng = R.N_NODES, np.random.default_rng([mode, H, C, seed])
    D = H * C
    inp = {k: rng.standard_normal((n, D)).astype(f32) for k in ("Q", "K", "V", "dout")}
    inp["F"] = rng.standard_normal((len(s), D)).astype(f32)
    inp["a"] = rng.standard_normal((H, C)).astype(f32)
    inp["bias"] = rng.standard_normal(D).astype(f32)
    if mode == GATV2:
        del inp["V"]
    scale = float(np.float32(np.sqrt(np.float32(C))))
    sh = lambda k: None if k not in inp else inp[k].astype(f64).reshape(-1, H, C)      # noqa: E731
    o, c = R.core(MODE_NAME[mode], s, t, n, sh("Q"), sh("K"), sh("V"), sh("F"), inp["a"].astype(f64), SLOPE, scale)
    stats = np.stack([c["m"], c["den"]], axis=-1)
    inp["stats"] = stats.astype(f32)
    gr = R.core_grad(MODE_NAME[mode], s, t, n, sh("Q"), sh("K"), sh("V"), sh("F"), inp["a"].astype(f64), SLOPE, scale, c, sh("dout"))
    grad = {k: v.reshape(v.shape[0], D) for k, v in gr.items() if k in ("dQ", "dK", "dV", "dF", "dA")}
    if mode == GATV2:
        grad["da"] = gr["da"]
    out = np.where(o.reshape(n, D) + inp["bias"] < 0, 0.0, o.reshape(n, D) + inp["bias"])      # act = relu
    return dict(inp=inp, fwd=dict(out=out, stats=stats), grad=grad, scale=scale, E=len(s), n=n)


def fwd_arrays(case):
    i = case["inp"]
    arrs = [A.Arr(k, "in", i[k]) for k in ("Q", "K", "V", "F", "a", "bias") if k in i]
    return arrs + [A.Arr("out", "out", shape=i["Q"].shape), A.Arr("stats", "out", shape=i["stats"].shape)]


def grad_arrays(case, mode):
    i = case["inp"]
    n, D = i["Q"].shape
    arrs = [A.Arr(k, "in", i[k]) for k in ("Q", "K", "V", "F", "a", "stats", "dout") if k in i]
    arrs += [A.Arr("line", "scratch", shape=(n, i["stats"].shape[1], 4)), A.Arr("dQ", "out", shape=(n, D)), A.Arr("dK", "out", shape=(n, D))]
    arrs += [A.Arr("dV", "out", shape=(n, D))] if mode == DOT else [A.Arr("dA", "out", shape=(n, D)), A.Arr("da", "out", shape=i["a"].shape)]
    return arrs + [A.Arr("dF", "out", shape=i["F"].shape)]


def _p(slab):
    return lambda nm: slab.ptr(nm) if nm in slab.arrs and slab.arrs[nm].nbytes > 0 else None


def call_fwd(lib, plan, mode, slab, case, H, C, stream=None, act=1):
    from gnnmp import _lib
    p = _p(slab)
    job = _lib.AttnEdgeJob(p("Q"), p("K"), p("V"), p("F"), p("a"), p("bias"), p("out"), p("stats"), SLOPE, case["scale"], act)
    return lib.gnnmp_attn_conv_edge_f32(plan, mode, ctypes.byref(job), H, C, stream)


def call_grad(lib, plan, plan_t, mode, slab, case, H, C, stream=None):
    from gnnmp import _lib
    p = _p(slab)
    job = _lib.AttnEdgeGradJob(p("Q"), p("K"), p("V"), p("F"), p("a"), p("stats"), p("dout"), p("line"), p("dQ"), p("dK"), p("dV"), p("dF"),
                               p("dA"), p("da"), SLOPE, case["scale"])
    return lib.gnnmp_attn_conv_edge_grad_f32(plan, plan_t, mode, ctypes.byref(job), H, C, stream)


def grad_want(case):
    """a difference of float64 terms may cancel to exactly zero (α (g − D) on the one-edge row): the floor is the scale of the terms"""
    return {k: A.E(v, scale=float(np.abs(v).max())) for k, v in case["grad"].items()}


def contract_graph(E=None):
    s, t = R.graph()
    if E is not None:
        s, t = s[:E], t[:E]
    return A.Graph("attn_edge", s + 1, t + 1, R.N_NODES)


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU 1: the raw exports — memory contract, alignment, E = 0, capture, determinism
# ------------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("mode", [GATV2, DOT], ids=["gatv2", "dot"])
@pytest.mark.parametrize("H,C", WIDTHS + [(4, 32)])
def test_memory_contract_of_the_exports(lib, mode, H, C):
    """every element of out, stats, dQ, dK, dV, dF (all E rows), dA, da written and right, nothing outside them touched, with each
    [.][H*C] array in turn shifted to 16-, 8- and 4-byte alignment, on a side stream.  (4, 32): 128 floats are 32 lanes of 4 and 64 lanes
    of 2, and with a 4-byte-aligned array 128 lanes of 1 — GNNMP_EUNSUPPORTED, as the header says, and nothing written"""
    import torch
    side = torch.cuda.Stream()
    sp = ctypes.c_void_p(side.cuda_stream)
    plans = A.Plans(lib)
    g = contract_graph()
    case = core_case(mode, H, C)
    wide = H * C > 64
    try:
        plan, plan_t = plans.get(A.Pl(g)), plans.get(A.Pl(g, T=True))
        for arrays, call, want, vec_arrays in (
                (fwd_arrays(case), lambda slab: call_fwd(lib, plan, mode, slab, case, H, C, sp), dict(case["fwd"]), ("Q", "K", "V", "F", "out")),
                (grad_arrays(case, mode), lambda slab: call_grad(lib, plan, plan_t, mode, slab, case, H, C, sp), grad_want(case),
                 ("Q", "K", "V", "F", "dout", "dQ", "dK", "dV", "dA", "dF"))):
            names = [a.name for a in arrays if a.name in vec_arrays]
            if wide:
                names = names[:2] + names[-2:]
            runs = [{}] + [{nm: A.SHIFTS[al]} for nm in names for al in ("a16", "a8", "a4")]
            for shifts in runs:
                slab = A.Slab(arrays, "cuda", shifts)
                torch.cuda.synchronize()
                rc = call(slab)
                torch.cuda.synchronize()
                if wide and 4 in shifts.values():
                    assert rc == A.EUNSUPPORTED, (shifts, rc)
                    assert not slab.check({}, untouched=True), shifts
                    continue
                assert rc == A.OK, (shifts, lib.gnnmp_last_error())
                problems = slab.check(want)
                assert not problems, (shifts, problems)
    finally:
        plans.close()


@gpu
@pytest.mark.parametrize("mode", [GATV2, DOT], ids=["gatv2", "dot"])
def test_no_edges(lib, mode):
    """E = 0 with N > 0: out = act(bias), stats = (-Inf, 0); zero dQ, dK, dV (dA, da); F and dF are NULL and not touched"""
    import torch
    H, C = 2, 6
    case = core_case(mode, H, C, E=0)
    assert case["E"] == 0 and not case["grad"]["dQ"].any() and np.all(np.isneginf(case["fwd"]["stats"][..., 0]))
    plans = A.Plans(lib)
    g = contract_graph(E=0)
    try:
        plan, plan_t = plans.get(A.Pl(g)), plans.get(A.Pl(g, T=True))
        slab = A.Slab(fwd_arrays(case))
        assert call_fwd(lib, plan, mode, slab, case, H, C) == A.OK, lib.gnnmp_last_error()
        torch.cuda.synchronize()
        assert not slab.check(dict(case["fwd"]))
        slab = A.Slab(grad_arrays(case, mode))
        assert call_grad(lib, plan, plan_t, mode, slab, case, H, C) == A.OK, lib.gnnmp_last_error()
        torch.cuda.synchronize()
        want = {k: A.E(v, tol="exact") for k, v in case["grad"].items()}
        assert not slab.check(want)
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
@pytest.mark.parametrize("which", ["forward", "grad"])
@pytest.mark.parametrize("mode", [GATV2, DOT], ids=["gatv2", "dot"])
def test_the_exports_record_into_a_hip_graph_without_an_eager_call(lib, mode, which):
    """fresh plans, no eager call first; two replays with re-fed inputs, each equal to an eager call bit for bit"""
    H, C = 2, 6
    plans = A.Plans(lib)
    g = contract_graph()
    cases = [core_case(mode, H, C, seed) for seed in (100, 101)]
    try:
        plan, plan_t = plans.get(A.Pl(g)), plans.get(A.Pl(g, T=True))
        if which == "forward":
            slab = A.Slab(fwd_arrays(cases[0]))
            call = lambda sp: call_fwd(lib, plan, mode, slab, cases[0], H, C, sp)      # noqa: E731
            wants = [dict(c["fwd"]) for c in cases]
        else:
            slab = A.Slab(grad_arrays(cases[0], mode))
            call = lambda sp: call_grad(lib, plan, plan_t, mode, slab, cases[0], H, C, sp)      # noqa: E731
            wants = [grad_want(c) for c in cases]
        reloads = [{k: v for k, v in c["inp"].items() if k in slab.arrs and slab.arrs[k].role == "in"} for c in cases]
        assert not np.array_equal(reloads[0]["F"], reloads[1]["F"])
        _capture_and_replay(lib, slab, call, reloads, wants)
    finally:
        plans.close()


@gpu
@pytest.mark.parametrize("mode", [GATV2, DOT], ids=["gatv2", "dot"])
def test_two_calls_give_equal_bits(lib, mode):
    import torch
    H, C = 3, 4
    case = core_case(mode, H, C)
    plans = A.Plans(lib)
    g = contract_graph()
    try:
        plan, plan_t = plans.get(A.Pl(g)), plans.get(A.Pl(g, T=True))
        for arrays, call in ((fwd_arrays(case), lambda slab: call_fwd(lib, plan, mode, slab, case, H, C)),
                             (grad_arrays(case, mode), lambda slab: call_grad(lib, plan, plan_t, mode, slab, case, H, C))):
            outs = []
            for _ in range(2):
                slab = A.Slab(arrays)
                assert call(slab) == A.OK, lib.gnnmp_last_error()
                torch.cuda.synchronize()
                outs.append(slab.outputs())
            assert all(np.array_equal(outs[0][k], outs[1][k]) for k in outs[0])
    finally:
        plans.close()


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU 2: the layers — forward and gradient parity, with the e-less pullback as the control
# ------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def layer_case(kind, H, C, concat, root=True, skip=False, edge=True):
    """(x, e, params, r, y64, grads64) of one layer case; computed once and shared"""
    s, t = R.graph()
    n = R.N_NODES
    rng = np.random.default_rng([1 if kind == "gatv2" else 2, H, C, int(concat), int(root), int(skip)])
    om = C * (H if concat else 1)
    cin = om if skip else 5
    x = rng.standard_normal((n, cin)).astype(f32)
    e = rng.standard_normal((len(s), EIN)).astype(f32)
    r = rng.standard_normal((n, om)).astype(f32)
    if kind == "gatv2":
        p = R.gatv2_params(rng, cin, EIN, H, C, concat, "relu", edge)
        y, _ = R.gatv2_layer(s, t, n, x, e, p)
        g = R.gatv2_grad(s, t, n, x, e, p, r)
    else:
        p = R.transformer_params(rng, cin, EIN, H, C, concat, root, skip, edge)
        y, _ = R.transformer_layer(s, t, n, x, e, p)
        g = R.transformer_grad(s, t, n, x, e, p, r)
    return x, e, p, r, y, g


def make_gatv2(p, cin):
    from gnnmp.layers_attn import GATv2Conv
    C = p["Wi"].shape[0] // p["H"]
    ch = ((cin, EIN), C) if p["We"] is not None else (cin, C)
    l = GATv2Conv(ch, "relu", heads=p["H"], concat=p["concat"], negative_slope=p["slope"], add_self_loops=False)
    for name, key in (("dense_i_weight", "Wi"), ("dense_i_bias", "bi"), ("dense_j_weight", "Wj"), ("dense_e_weight", "We"), ("a", "a"),
                      ("bias", "bias")):
        if p[key] is not None:
            assert tuple(getattr(l, name).shape) == p[key].shape, name
            setattr(l, name, dev(p[key]).requires_grad_(True))
    return l


def make_transformer(p, cin):
    from gnnmp.layers_attn import TransformerConv
    C = p["W2"].shape[0] // p["H"]
    ch = ((cin, EIN), C) if p["W6"] is not None else (cin, C)
    l = TransformerConv(ch, heads=p["H"], concat=p["concat"], root_weight=p["W1"] is not None, skip_connection=p["skip"])
    for k in ("1", "2", "3", "4", "6"):
        for name, key in (("W%s_weight" % k, "W" + k), ("W%s_bias" % k, "b" + k)):
            if p[key] is not None:
                assert tuple(getattr(l, name).shape) == p[key].shape, name
                setattr(l, name, dev(p[key]).requires_grad_(True))
    return l


GAT_GRADS = (("dense_i_weight", "dWi"), ("dense_i_bias", "dbi"), ("dense_j_weight", "dWj"), ("dense_e_weight", "dWe"), ("a", "da"),
             ("bias", "dbias"))
TR_GRADS = tuple(("W%s_weight" % k, "dW" + k) for k in "12346") + tuple(("W%s_bias" % k, "db" + k) for k in "12346")


def _layer_check(kind, l, g, case, fwd, ad, names, tag):
    """forward through the layer call and through *_ad, then every gradient; returns the worst gradient ratio"""
    x, e, p, r, y64, g64 = case
    edge = (p["We"] if kind == "gatv2" else p["W6"]) is not None
    xt, et = dev(x).requires_grad_(True), dev(e).requires_grad_(True) if edge else None
    close(fwd(l, g, dev(x), dev(e) if edge else None), y64, f"{tag} forward")
    y = ad(l, g, xt, et) if edge else ad(l, g, xt)
    close(y, y64, f"{tag} forward (ad)")
    (y * dev(r)).sum().backward()
    worst = close(xt.grad, g64["dx"], f"{tag} dx")
    if edge:
        worst = max(worst, close(et.grad, g64["de"], f"{tag} de"))
    for name, key in names:
        param = getattr(l, name)
        if param is None:
            assert g64[key] is None, name
            continue
        assert param.grad is not None, name
        worst = max(worst, close(param.grad, g64[key], f"{tag} {key}"))
    print(f"{tag}: worst gradient ratio {worst:.3e}")
    return worst


@gpu
@pytest.mark.parametrize("concat", [True, False], ids=["concat", "mean"])
@pytest.mark.parametrize("H,C", WIDTHS)
def test_gatv2_with_edge_features_against_float64(graph, H, C, concat):
    """gatv2_conv / gatv2_conv_ad with e: forward, dx, de and every weight at 1e-5 (norm-wise), and the e-less layer on the same graph
    under the same measure as the control"""
    from gnnmp.backward_attn import gatv2_conv_ad
    from gnnmp.layers_attn import gatv2_conv
    g, s, t = graph
    case = layer_case("gatv2", H, C, concat)
    edge = _layer_check("gatv2", make_gatv2(case[2], case[0].shape[1]), g, case, gatv2_conv, gatv2_conv_ad, GAT_GRADS, f"gatv2 e ({H},{C})")
    ctrl = layer_case("gatv2", H, C, concat, edge=False)
    control = _layer_check("gatv2", make_gatv2(ctrl[2], ctrl[0].shape[1]), g, ctrl, lambda l, g_, x, e: gatv2_conv(l, g_, x), gatv2_conv_ad,
                           GAT_GRADS, f"gatv2 control ({H},{C})")
    print(f"MEASURED gatv2 ({H},{C}) concat={concat}: edge {edge:.3e} control {control:.3e}")


@gpu
@pytest.mark.parametrize("root,skip", [(True, False), (False, True)], ids=["root", "skip"])
@pytest.mark.parametrize("concat", [True, False], ids=["concat", "mean"])
@pytest.mark.parametrize("H,C", WIDTHS)
def test_transformer_with_edge_features_against_float64(graph, H, C, concat, root, skip):
    from gnnmp.backward_attn import transformer_conv_ad
    from gnnmp.layers_attn import transformer_conv
    g, s, t = graph
    case = layer_case("transformer", H, C, concat, root, skip)
    edge = _layer_check("transformer", make_transformer(case[2], case[0].shape[1]), g, case, transformer_conv, transformer_conv_ad, TR_GRADS,
                        f"transformer e ({H},{C})")
    ctrl = layer_case("transformer", H, C, concat, root, skip, edge=False)
    control = _layer_check("transformer", make_transformer(ctrl[2], ctrl[0].shape[1]), g, ctrl,
                           lambda l, g_, x, e: transformer_conv(l, g_, x), transformer_conv_ad, TR_GRADS, f"transformer control ({H},{C})")
    print(f"MEASURED transformer ({H},{C}) concat={concat} root={root} skip={skip}: edge {edge:.3e} control {control:.3e}")


@gpu
def test_zero_edge_weights_agree_with_the_e_less_layer(graph):
    """dense_e_weight = 0 / W6 = 0: the edge path computes the e-less layer, to the forward bar"""
    import torch
    from gnnmp.layers_attn import gatv2_conv, transformer_conv
    g, s, t = graph
    x, e, p, *_ = layer_case("gatv2", 2, 6, True)
    l, l0 = make_gatv2(p, x.shape[1]), make_gatv2(dict(p, We=None), x.shape[1])
    l.dense_e_weight = torch.zeros_like(l.dense_e_weight)
    close(gatv2_conv(l, g, dev(x), dev(e)), gatv2_conv(l0, g, dev(x)).detach().cpu().numpy().astype(f64), "gatv2, dense_e = 0")
    x, e, p, *_ = layer_case("transformer", 2, 6, True)
    l, l0 = make_transformer(p, x.shape[1]), make_transformer(dict(p, W6=None, b6=None), x.shape[1])
    l.W6_weight, l.W6_bias = torch.zeros_like(l.W6_weight), None
    close(transformer_conv(l, g, dev(x), dev(e)), transformer_conv(l0, g, dev(x)).detach().cpu().numpy().astype(f64), "transformer, W6 = 0")


@gpu
def test_needs_input_grad_prunes(graph):
    """what nobody asks for is not computed: e and the edge weights without requires_grad get no gradient, the others keep their bits"""
    import torch
    from gnnmp.backward_attn import gatv2_conv_ad, transformer_conv_ad
    g, s, t = graph
    for kind, make, ad, wname in (("gatv2", make_gatv2, gatv2_conv_ad, "dense_e_weight"), ("transformer", make_transformer, transformer_conv_ad, "W6_weight")):
        x, e, p, r, *_ = layer_case(kind, 2, 6, True)
        full, part = make(p, x.shape[1]), make(p, x.shape[1])
        setattr(part, wname, getattr(part, wname).detach())
        xs = []
        for l, e_grad in ((full, True), (part, False)):
            xt, et = dev(x).requires_grad_(True), dev(e).requires_grad_(e_grad)
            (ad(l, g, xt, et) * dev(r)).sum().backward()
            xs.append(xt.grad)
            assert (et.grad is not None) == e_grad
        assert getattr(part, wname).grad is None and getattr(full, wname).grad is not None
        assert torch.equal(xs[0], xs[1])


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU 3: the e-less paths run the calls they ran before; the host's refusals
# ------------------------------------------------------------------------------------------------------------------------------------
@gpu
def test_layers_without_ein_are_untouched_bit_for_bit(lib, graph):
    """a layer built without ein goes through gnnmp_attn_conv_f32 / gnnmp_attn_conv_grad_f32 as before: layer call, *_ad forward and the
    gradients equal direct calls of those exports bit for bit"""
    import torch
    from gnnmp import _lib as L
    from gnnmp.backward import act_grad, dense_grad_x
    from gnnmp.backward_attn import gatv2_conv_ad, transformer_conv_ad
    from gnnmp.layers import dense
    from gnnmp.layers_attn import GATv2Conv, TransformerConv, gatv2_conv, transformer_conv
    g, s, t = graph
    n, H, C, cin = R.N_NODES, 2, 6, 5
    x = dev(np.random.default_rng(5).standard_normal((n, cin)).astype(f32))
    r = dev(np.random.default_rng(6).standard_normal((n, H * C)).astype(f32))
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device="cuda")      # noqa: E731
    sp = L.stream_ptr()

    def direct(loops, mode, Q, K, V, a, scale, bias, act):
        plan, plan_t = g.plan(loops), g.plan_transposed(loops)
        out, stats = new(n, H * C), new(n, H, 2)
        L.check(lib.gnnmp_attn_conv_f32(plan.handle, mode, ptr(Q), ptr(K), ptr(V), ptr(a), SLOPE, scale, ptr(bias), act, ptr(out), ptr(stats),
                                        H, C, sp))
        dz = act_grad(r, out, "relu") if act else r
        line, dQ, dK, dV, dA, da = new(n, H, 4), new(n, H * C), new(n, H * C), new(n, H * C), new(n, H * C), new(H, C)
        L.check(lib.gnnmp_attn_conv_grad_f32(plan.handle, plan_t.handle, mode, ptr(Q), ptr(K), ptr(V), ptr(a), SLOPE, scale, ptr(stats),
                                             ptr(dz), ptr(line), ptr(dQ), ptr(dK), ptr(dV) if mode == DOT else None,
                                             ptr(dA) if mode == GATV2 else None, ptr(da) if mode == GATV2 else None, H, C, sp))
        return out, dQ, dK, dV, da

    l = GATv2Conv((cin, C), "relu", heads=H, seed=3)                        # add_self_loops = true, the default
    l.bias = dev(np.random.default_rng(7).standard_normal(H * C).astype(f32))
    assert l.dense_e_weight is None
    Q, K = dense(x, l.dense_i_weight, l.dense_i_bias), dense(x, l.dense_j_weight)
    out, dQ, dK, _, da = direct(True, GATV2, Q, K, None, l.a_hc, 1.0, l.bias, 1)
    assert torch.equal(gatv2_conv(l, g, x), out)
    xt = x.clone().requires_grad_(True)
    l.a.requires_grad_(True)
    y = gatv2_conv_ad(l, g, xt)
    assert torch.equal(y.detach(), out)
    (y * r).sum().backward()
    dx = dense_grad_x(dQ, l.dense_i_weight)
    L.check(lib.gnnmp_add_f32(ptr(dx), ptr(dense_grad_x(dK, l.dense_j_weight)), ptr(dx), dx.numel(), sp))
    assert torch.equal(xt.grad, dx) and torch.equal(l.a.grad, da.t())

    tr = TransformerConv((cin, C), heads=H, root_weight=False, seed=4)
    assert tr.W6_weight is None
    V, Q, K = dense(x, tr.W2_weight, tr.W2_bias), dense(x, tr.W3_weight, tr.W3_bias), dense(x, tr.W4_weight, tr.W4_bias)
    out, dQ, dK, dV, _ = direct(False, DOT, Q, K, V, None, tr.sqrt_out, None, 0)
    assert torch.equal(transformer_conv(tr, g, x), out)
    xt = x.clone().requires_grad_(True)
    y = transformer_conv_ad(tr, g, xt)
    assert torch.equal(y.detach(), out)
    (y * r).sum().backward()
    dx = dense_grad_x(dV, tr.W2_weight)
    for d, W in ((dQ, tr.W3_weight), (dK, tr.W4_weight)):
        L.check(lib.gnnmp_add_f32(ptr(dx), ptr(dense_grad_x(d, W)), ptr(dx), dx.numel(), sp))
    assert torch.equal(xt.grad, dx)


@gpu
def test_host_refusals(graph):
    """the reference's assertions (e missing, e undeclared; ein with self loops is the constructor's: tested without a GPU), a wrong edge
    count, and this path's own refusals by name — dropout with e, a row wider than a wave — before any C call"""
    import torch
    from gnnmp.backward_attn import gatv2_conv_ad, transformer_conv_ad
    from gnnmp.layers_attn import GATv2Conv, TransformerConv, gatv2_conv, transformer_conv
    g, s, t = graph
    n, E = R.N_NODES, len(s)
    x, e = torch.zeros((n, 5), device="cuda"), torch.zeros((E, EIN), device="cuda")
    with_e = (GATv2Conv(((5, EIN), 4), heads=2, add_self_loops=False), TransformerConv(((5, EIN), 4), heads=2))
    without = (GATv2Conv((5, 4), heads=2, add_self_loops=False), TransformerConv((5, 4), heads=2))
    calls = ((gatv2_conv, gatv2_conv_ad), (transformer_conv, transformer_conv_ad))
    for l, l0, fns in zip(with_e, without, calls):
        for fn in fns:
            with pytest.raises(AssertionError, match="Input edge features required for this layer"):
                fn(l, g, x)
            with pytest.raises(AssertionError, match="Input edge features were not specified in the layer constructor"):
                fn(l0, g, x, e)
            with pytest.raises(AssertionError, match="edges"):
                fn(l, g, x, e[:-1])
    wide = (GATv2Conv(((5, EIN), 65), heads=1, add_self_loops=False), TransformerConv(((5, EIN), 13), heads=5))
    for l, fns in zip(wide, calls):
        for fn in fns:
            with pytest.raises(AssertionError, match="must fit one wave"):
                fn(l, g, x, e)
    drop = GATv2Conv(((5, EIN), 4), heads=2, add_self_loops=False, dropout=0.25)
    for fn in calls[0]:
        with pytest.raises(AssertionError, match="dropout together with edge features"):
            fn(drop, g, x, e)
    loops = GATv2Conv((5, 4), heads=2)                        # self loops, no ein: e is refused as undeclared
    with pytest.raises(AssertionError):
        gatv2_conv(loops, g, x, e)
