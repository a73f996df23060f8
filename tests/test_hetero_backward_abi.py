"""The heterograph adjoints without a GPU: gnnmp_hetero_propagate_grad_f32 exists in header, SYMBOLS and library; its ctypes records have
the C layout; every bad argument is refused with its status before any HIP call; the float64 restatement the GPU tests compare against
(tests/hetero_grad_ref.py) agrees with central finite differences of the forward restatement (tests/hetero_ref.py); and the Python
adjoints refuse what they do not cover before any device call."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hetero_grad_ref as G  # noqa: E402
import hetero_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "gnnmp_hetero_propagate_grad_f32"


def test_header_symbols_and_library_carry_the_export():
    import gnnmp
    from gnnmp import _lib
    header = open(os.path.join(ROOT, "include", "gnnmp.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert f"int {NAME}(const gnnmp_hetero_src_t *srcs, int n_srcs, int64_t D, gnnmp_stream_t stream);" in header
    assert "} gnnmp_hetero_rel_grad_t;" in header and "} gnnmp_hetero_src_t;" in header
    assert NAME in _lib.SYMBOLS
    assert NAME in {line.split()[-1] for line in nm.splitlines() if line.strip()}
    for name in ("hetero_propagate_grad", "hetero_propagate_ad", "hetero_conv_ad"):
        assert hasattr(gnnmp, name), name


def test_the_ctypes_records_have_the_header_layout():
    """gnnmp_hetero_rel_grad_t {plan_t, dy, w, sd, y, out} and gnnmp_hetero_src_t {dx, x, n_src, n_rel, rels} as a C compiler lays them
    out (LP64)"""
    from gnnmp import _lib
    assert ctypes.sizeof(_lib.HeteroRelGrad) == 48
    assert [getattr(_lib.HeteroRelGrad, f).offset for f in ("plan_t", "dy", "w", "sd", "y", "out")] == [0, 8, 16, 24, 32, 40]
    assert ctypes.sizeof(_lib.HeteroSrc) == 40
    assert [getattr(_lib.HeteroSrc, f).offset for f in ("dx", "x", "n_src", "n_rel", "rels")] == [0, 8, 16, 24, 32]


P = lambda v: ctypes.c_void_p(0x1000 * v) if v else None      # never dereferenced: the call must refuse first  # noqa: E731


def _call(lib, n_srcs=1, D=4, dx=1, x=2, n_src=5, n_rel=1, rels=True, plan_t=None, dy=3, w=None, sd=None, y=None, out=None, null_table=False):
    from gnnmp import _lib
    tab = (_lib.HeteroRelGrad * max(n_rel, 1))()
    for r in tab:
        r.plan_t, r.dy, r.w, r.sd, r.y, r.out = plan_t, P(dy), P(w), P(sd), P(y), P(out)
    srcs = (_lib.HeteroSrc * max(n_srcs, 1))()
    for s in srcs:
        s.dx, s.x, s.n_src, s.n_rel = P(dx), P(x), n_src, n_rel
        s.rels = tab if rels else ctypes.POINTER(_lib.HeteroRelGrad)()
    return lib.gnnmp_hetero_propagate_grad_f32(None if null_table else srcs, n_srcs, D, None)


class _FakePlan(ctypes.Structure):
    """the head of csrc/common.h's gnnmp_graph {int64 n_src, n_dst, n_edges, n_total; ...}: all the refusals read of a plan.  The tail is
    zeroed room for the pointers the call would copy (never dereference) if it did not refuse."""
    _fields_ = [("n_src", ctypes.c_int64), ("n_dst", ctypes.c_int64), ("n_edges", ctypes.c_int64), ("n_total", ctypes.c_int64),
                ("tail", ctypes.c_char * 1024)]


def test_argument_validation_needs_no_gpu():
    """every refusal comes before the first HIP call: this test runs on a machine without a device, on pointers that are not memory"""
    from gnnmp import _lib
    lib = _lib.load()
    EINVAL, cap = _lib.EINVAL, _lib.HETERO_MAX_REL
    assert _call(lib, null_table=True) == EINVAL and b"source table" in lib.gnnmp_last_error()
    assert _call(lib, n_srcs=0) == EINVAL
    assert _call(lib, rels=False) == EINVAL and b"relation table" in lib.gnnmp_last_error()
    assert _call(lib, n_rel=0) == EINVAL
    assert _call(lib, D=0) == EINVAL and b"bad D" in lib.gnnmp_last_error()
    assert _call(lib, D=-4) == EINVAL
    assert _call(lib, D=(1 << 20) + 1) == EINVAL
    assert _call(lib, dx=None) == EINVAL and b"null dx" in lib.gnnmp_last_error()
    assert _call(lib, dy=None) == EINVAL and b"null dy" in lib.gnnmp_last_error()
    assert _call(lib, n_src=-1) == EINVAL
    assert _call(lib, n_src=2**31) == EINVAL
    assert _call(lib, out=4) == EINVAL and b"out without y" in lib.gnnmp_last_error()
    assert _call(lib, y=4) == EINVAL and b"needs out" in lib.gnnmp_last_error()
    # records with a plan: a transposed plan of 5 rows and 7 slots
    plan = _FakePlan(n_src=9, n_dst=5, n_edges=7, n_total=7)
    pp = ctypes.addressof(plan)
    assert _call(lib, plan_t=pp, y=4, w=5) == EINVAL and b"together with w or sd" in lib.gnnmp_last_error()
    assert _call(lib, plan_t=pp, y=4, sd=5) == EINVAL and b"together with w or sd" in lib.gnnmp_last_error()
    assert _call(lib, plan_t=pp, y=4, out=5) == EINVAL and b"identity relations" in lib.gnnmp_last_error()
    assert _call(lib, plan_t=pp, y=4, x=None) == EINVAL and b"null x" in lib.gnnmp_last_error()
    assert _call(lib, plan_t=pp, dy=None) == EINVAL and b"null dy" in lib.gnnmp_last_error()
    assert _call(lib, plan_t=pp, n_src=6) == EINVAL and b"the transposed plan has 5 rows, the table 6 sources" in lib.gnnmp_last_error()
    # more relations than the cap, in one source type or over several
    assert _call(lib, n_rel=cap + 1) == _lib.EUNSUPPORTED and str(cap).encode() in lib.gnnmp_last_error()
    assert _call(lib, n_srcs=3, n_rel=cap // 2) == _lib.EUNSUPPORTED
    assert _call(lib, n_srcs=cap + 1) == _lib.EUNSUPPORTED


def test_a_call_without_rows_is_accepted_and_launches_nothing():
    """n_src = 0 everywhere: every pointer may be NULL, no block is launched, the status is OK — on a machine without a device"""
    from gnnmp import _lib
    lib = _lib.load()
    assert _call(lib, n_src=0, dx=None, x=None, dy=None) == _lib.OK
    assert _call(lib, n_srcs=2, n_src=0, n_rel=_lib.HETERO_MAX_REL // 2) == _lib.OK
    plan = _FakePlan(n_src=9, n_dst=0, n_edges=0, n_total=0)
    assert _call(lib, n_src=0, plan_t=ctypes.addressof(plan), dx=None, x=None, dy=None) == _lib.OK


def test_python_adjoints_refuse_before_the_device():
    """an unsupported σ (via _act_code) and max with edge weights raise ValueError before any device call: no GPU is needed to see them"""
    import torch
    import gnnmp
    from gnnmp import backward_hetero

    class Member(gnnmp.GraphConv):          # a GraphConv without touching the device
        def __init__(self, sigma):
            self.sigma, self.aggr, self.bias = sigma, "+", None
            self.weight1 = self.weight2 = torch.zeros((2, 2))

    class Graph:                             # hetero_propagate_ad reads these before it touches the device
        etypes = [("A", "to", "B")]
        device = "cpu"
        graph = {("A", "to", "B"): (None, None, None)}

        def num_edges_of(self, et):
            return 3

    et = ("A", "to", "B")
    for sigma in (torch.tanh, torch.sigmoid):
        with pytest.raises(ValueError, match="identity and relu"):
            gnnmp.hetero_conv_ad(gnnmp.HeteroGraphConv({et: Member(sigma)}), Graph(), {})
    with pytest.raises(ValueError, match="unsupported activation"):
        gnnmp.hetero_conv_ad(gnnmp.HeteroGraphConv({et: Member("softplus")}), Graph(), {})
    with pytest.raises(NotImplementedError, match="object"):
        gnnmp.hetero_conv_ad(gnnmp.HeteroGraphConv({et: object()}), Graph(), {})
    for op in ("max", "min"):
        with pytest.raises(ValueError, match="no edge weights"):
            gnnmp.hetero_propagate_ad(Graph(), {}, aggr=op, edge_weight={et: torch.ones(3)})
    with pytest.raises(ValueError, match="combine"):
        gnnmp.hetero_propagate_ad(Graph(), {}, combine="mean")
    assert backward_hetero._act_code("relu") == 1 and backward_hetero._act_code(None) == 0


# ---- the float64 restatement against central finite differences -------------------------------------------------------------------------
# a 3-type, 4-relation graph, D = 3: B receives from A twice (one relation weighted) and from C, A receives from B
ETS = [("A", "ab", "B"), ("C", "cb", "B"), ("B", "ba", "A"), ("A", "ab2", "B")]
NUM = {"A": 6, "B": 5, "C": 4}
D, H, TOL = 3, 1e-6, 1e-6
SEED, CONV_SEED = 5, 4      # picked so that the set-ups' own assertions (no kink within the step) hold in every case


def _edges(rng, n_src, n_dst, m, extremal):
    """(s, t) of a relation.  + / mean: m random edges, some destinations stay without one, repeated edges allowed.  max / min: every
    destination has one to three DISTINCT sources — an empty row's ∓Inf has no derivative, and a repeated edge is a tie with itself
    (NNlib's rule hands Δ to each copy; the function's derivative counts it once)"""
    if not extremal:
        return rng.integers(0, n_src, m), rng.integers(0, n_dst, m)
    pairs = [(j, i) for i in range(n_dst) for j in rng.choice(n_src, rng.integers(1, 4), replace=False)]
    pairs = [pairs[k] for k in rng.permutation(len(pairs))]
    return np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs])


def _setup(aggrs, weighted, combine):
    """the graph, inputs and cotangents; asserts that every max / min in play — a relation's, and the fold's — has its candidates more
    than 1e-3 apart, so that a step of 1e-6 crosses no kink"""
    rng = np.random.default_rng(SEED)
    coo = {et: _edges(rng, NUM[et[0]], NUM[et[2]], 7 + k, aggrs[et] in ("max", "min")) for k, et in enumerate(ETS)}
    x = {k: rng.uniform(-1, 1, (n, D)) for k, n in NUM.items()}
    w = {et: rng.uniform(0.5, 1.5, len(coo[et][0])) if et in weighted else None for et in ETS}
    root = {k: rng.uniform(-1, 1, (NUM[k], D)) for k in ("A", "B")}
    dout = {k: rng.uniform(-1, 1, (NUM[k], D)) for k in ("A", "B")}
    for et in ETS:
        if aggrs[et] in ("max", "min"):
            s, t = coo[et]
            for i in range(NUM[et[2]]):
                c = np.sort(x[et[0]][np.unique(s[t == i])], axis=0)
                assert c.shape[0] < 2 or np.diff(c, axis=0).min() > 1e-3, "competing candidates of a max / min relation too close"
    if combine != "+":
        for dst in ("A", "B"):
            terms = [root[dst]] + [R.propagate_ref(*coo[et], NUM[dst], x[et[0]], w[et], aggrs[et], np.float64) for et in ETS if et[2] == dst]
            c = np.sort(np.stack(terms), axis=0)
            c = c[:, np.isfinite(c).all(axis=0)]
            assert np.diff(c, axis=0).min() > 1e-3, "competing terms of the fold too close"
    return coo, x, w, root, dout


def _forward_loss(coo, x, w, root, dout, aggrs, combine):
    loss = 0.0
    for dst in ("A", "B"):
        rels = [(coo[et][0], coo[et][1], x[et[0]], w[et], aggrs[et]) for et in ETS if et[2] == dst]
        out = R.hetero_ref(rels, NUM[dst], combine, np.float64, root=root[dst])
        loss += float((out * dout[dst]).sum())
    return loss


def _fd(f, arr):
    """central differences of f() w.r.t. every element of arr (perturbed in place, restored) — no element is skipped"""
    g = np.zeros_like(arr)
    for i in np.ndindex(arr.shape):
        keep = arr[i]
        arr[i] = keep + H
        hi = f()
        arr[i] = keep - H
        lo = f()
        arr[i] = keep
        g[i] = (hi - lo) / (2 * H)
    return g


def _agree(fd, g, what):
    assert fd.shape == g.shape, what
    assert np.abs(fd - g).max() <= TOL * max(np.abs(g).max(), 1.0), f"{what}: {np.abs(fd - g).max():.3e}"


CASES = [
    ("+", {}, (), "+"), ("mean", {}, (), "+"), ("max", {}, (), "+"), ("min", {}, (), "+"),
    ("+", {ETS[1]: "mean", ETS[3]: "max"}, (ETS[0], ETS[1]), "+"),
    ("+", {ETS[1]: "mean", ETS[2]: "min"}, (ETS[0], ETS[1]), "max"),
    ("mean", {ETS[3]: "max"}, (ETS[0],), "min"),
]


@pytest.mark.parametrize("base,over,weighted,combine", CASES)
def test_float64_restatement_agrees_with_finite_differences(base, over, weighted, combine):
    aggrs = {et: over.get(et, base) for et in ETS}
    coo, x, w, root, dout = _setup(aggrs, weighted, combine)
    f = lambda: _forward_loss(coo, x, w, root, dout, aggrs, combine)      # noqa: E731
    dx = {k: np.zeros_like(v) for k, v in x.items()}
    droot, dw = {}, {}
    for dst in ("A", "B"):
        ets = [et for et in ETS if et[2] == dst]
        rels = [(coo[et][0], coo[et][1], x[et[0]], w[et], aggrs[et]) for et in ets]
        droot[dst], res = G.hetero_grad_ref(rels, NUM[dst], dout[dst], combine, root=root[dst])
        for et, (dxr, dwr) in zip(ets, res):
            dx[et[0]] += dxr
            dw[et] = dwr
    for k in x:
        _agree(_fd(f, x[k]), dx[k], f"Δx[{k}]")
    for k in root:
        _agree(_fd(f, root[k]), droot[k], f"Δroot[{k}]")
    for et in weighted:
        _agree(_fd(f, w[et]), dw[et], f"Δw[{et}]")
    assert all(dw[et] is None for et in ETS if et not in weighted)
    assert not dx["C"].any() or any(et[0] == "C" for et in ETS)


@pytest.mark.parametrize("sigma", [None, "relu"])
@pytest.mark.parametrize("aggr", ["+", "mean", "max"])
@pytest.mark.parametrize("combine", ["+", "max"])
def test_float64_conv_model_agrees_with_finite_differences(combine, aggr, sigma):
    """the numpy model of hetero_conv_ad's gradients (derived from hetero_conv_ref) against central differences of hetero_conv_ref"""
    rng = np.random.default_rng(CONV_SEED)
    # every destination has an edge in every relation (no ∓Inf aggregate under max), no edge twice
    coo = {et: _edges(rng, NUM[et[0]], NUM[et[2]], 0, True) for et in ETS}
    x = {k: rng.uniform(-1, 1, (n, D)) for k, n in NUM.items()}
    Dout = 2
    layers = [(et, (rng.uniform(-1, 1, (Dout, D)), rng.uniform(-1, 1, (Dout, D)), rng.uniform(-1, 1, Dout), sigma, aggr)) for et in ETS]
    dout = {k: rng.uniform(-1, 1, (NUM[k], Dout)) for k in ("A", "B")}
    # no kink within the step: candidates of max apart, pre-activations away from 0, competing layer outputs apart
    if aggr == "max":
        for et in ETS:
            s, t = coo[et]
            for i in range(NUM[et[2]]):
                c = np.sort(x[et[0]][np.unique(s[t == i])], axis=0)
                assert c.shape[0] < 2 or np.diff(c, axis=0).min() > 1e-3
    lin = [(et, p[:3] + (None, aggr)) for et, p in layers]
    for k, (et, _) in enumerate(layers):
        z = R.graph_conv_ref(*coo[et], NUM[et[2]], x[et[0]], x[et[2]], *lin[k][1])
        assert np.abs(z).min() > 1e-3, "a pre-activation too close to relu's kink"
    if combine == "max":
        ys = [R.graph_conv_ref(*coo[et], NUM[et[2]], x[et[0]], x[et[2]], *p) for et, p in layers if et[2] == "B"]
        gaps = np.diff(np.sort(np.stack(ys), axis=0), axis=0)
        assert gaps[gaps > 0].min() > 1e-3 and (sigma == "relu" or gaps.min() > 1e-3)

    def f():
        y = R.hetero_conv_ref(layers, coo, NUM, x, combine, np.float64)
        return sum(float((y[k] * dout[k]).sum()) for k in y)
    dx, dparams = G.hetero_conv_grad_ref(layers, coo, NUM, x, dout, combine)
    # (relu makes exact ties at 0 between layer outputs; every tying term receives Δ and relu' = 0 stops it there, as the differences see)
    for k in x:
        _agree(_fd(f, x[k]), dx[k], f"Δx[{k}]")
    for (et, (Wr, Wa, b, _, _)), (dWr, dWa, db) in zip(layers, dparams):
        _agree(_fd(f, Wr), dWr, f"ΔW_root {et}")
        _agree(_fd(f, Wa), dWa, f"ΔW_agg {et}")
        _agree(_fd(f, b), db, f"Δb {et}")
