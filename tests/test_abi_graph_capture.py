"""The ABI's no-sync, no-alloc rule (include/gnnmp.h, Conventions: compute entry points "launch on [the stream] and return; they never
call hipDeviceSynchronize and never allocate"), checked the way a caller relies on it: every export of the case table
(tests/abi_cases.py) is RECORDED into a HIP graph and REPLAYED.

  * a host wait or an allocation inside the call is an error under stream capture (capture_error_mode = "thread_local"), not a stall;
  * nothing may run while the call is recorded, and nothing may go to another stream: after the capture every output still holds the
    slab's poison;
  * a replay must give the bits of the eager call (the header's determinism rule: same kernel, same arguments, no float atomics);
  * new values copied over the inputs AT THE SAME ADDRESSES must give the new reference: a value read on the host at call time, or a
    cache keyed on a pointer, shows here;
  * two replays back to back, no host work between them, must give those bits again: arrival counters, tile tickets and set-aside
    lists have reset themselves on the device.

An export that waits or allocates is exempt only with the words of its own header comment that say so (A.SYNCHRONISES / A.ALLOCATES,
checked against the raw header without a GPU).  The layer level does the same with whole steps — forward, and forward + backward —
through the Python mirror.  References and bounds are those of the case table and of the per-layer tests (imported, not restated)."""
import os
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_cases as A  # noqa: E402

gpu = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------------------------------------------
# CPU: the classification against the header, the variants of the case table
# ------------------------------------------------------------------------------------------------------------------------------------
def _dry_ctx(variant=0):
    _, defines = A.parse_header()
    return A.Ctx(int(defines["GNNMP_MIN_LONG_ROW"]), variant=variant)


def _takes_plan(export):
    return any("gnnmp_graph_t" in p[3] for p in A.parse_header()[0][export])


def _capture_cases(ctx, export):
    """the cases section 2 records: the side-stream case, and for an export that takes a plan its workspace cases (hub graph: rows at,
    just above and five times above the plan's threshold)"""
    cs = A.TABLE[export](ctx)
    return [c for c in cs if "side" in c.tags or (_takes_plan(export) and "ws" in c.tags)]


def test_the_classes_partition_the_table():
    exempt = {**A.SYNCHRONISES, **A.ALLOCATES}
    assert not (set(A.SYNCHRONISES) & set(A.ALLOCATES))
    assert set(exempt) <= set(A.TABLE), set(exempt) - set(A.TABLE)
    assert set(A.capturable()) | set(exempt) == set(A.TABLE) and not (set(A.capturable()) & set(exempt))
    assert len(A.capturable()) > 60                         # the rule is the rule: the exemptions are a handful of graph-prep calls
    assert len(exempt) <= 8


@pytest.mark.parametrize("export", sorted({**A.SYNCHRONISES, **A.ALLOCATES}))
def test_an_exempt_export_is_quoted_from_its_own_header_comment(export):
    phrase = {**A.SYNCHRONISES, **A.ALLOCATES}[export]
    assert A.WAITS_OR_ALLOCATES.search(phrase), f"'{phrase}' does not say that {export} waits or allocates"
    want = " ".join(phrase.split())
    texts = A.header_comments_of(export)
    assert any(want in t for t in texts), f"the header's comment on {export} does not say '{want}': the export owes a capture case"


def test_a_silent_header_comment_cannot_be_quoted():
    """the condition that keeps the dict from hiding a failure: gnnmp_propagate_f32's comment says nothing of the kind, and the words of
    ANOTHER export's comment do not count for it"""
    assert not any(A.WAITS_OR_ALLOCATES.search(t) for t in A.header_comments_of("gnnmp_propagate_f32"))
    assert not any(A.WAITS_OR_ALLOCATES.search(t) for t in A.header_comments_of("gnnmp_gather_f32"))
    other = " ".join(A.SYNCHRONISES["gnnmp_rand_edge_split"].split())
    assert any(other in t for t in A.header_comments_of("gnnmp_rand_edge_split"))
    assert not any(other in t for t in A.header_comments_of("gnnmp_edge_dot_grad_f32"))      # same section comment, its own paragraph


def test_an_export_whose_own_comment_says_it_synchronises_is_not_captured():
    """the converse: the words "Synchronises the stream" / "Synchronisations:" in an export's own comment or paragraph put it in the dict"""
    says = [e for e in A.TABLE if any(("Synchronises the stream" in t or "Synchronisations:" in t) for t in A.header_comments_of(e))]
    assert sorted(says) == sorted(A.SYNCHRONISES), set(says) ^ set(A.SYNCHRONISES)


def _section_comment_of(export):
    """the whole section comment (the one ruled off with dashes) that governs an export: a sentence about "all of them" stands after
    the per-export paragraphs"""
    import re
    text = open(A.HEADER).read()
    at = re.search(r"\b%s\s*\(" % re.escape(export), re.sub(r"/\*.*?\*/", lambda c: " " * len(c.group(0)), text, flags=re.S)).start()
    sections = [c.group(0) for c in re.finditer(r"/\*.*?\*/", text, flags=re.S) if c.end() <= at and "-----" in c.group(0)]
    return " ".join(sections[-1].replace("*", " ").split()) if sections else ""


def test_a_case_is_recorded_cold_only_where_the_header_says_so():
    """no_warmup (the capture test then records the call without an eager call first) is a promise of the header, quoted here: the
    export's own comment or its section must say so; all cases of an export agree"""
    n = 0
    ctx = _dry_ctx()
    for export in A.capturable():
        cold = {c.no_warmup for c in A.TABLE[export](ctx)}
        assert len(cold) == 1, export
        if cold == {True}:
            texts = " ".join(A.header_comments_of(export)) + " " + _section_comment_of(export)
            assert "without an eager call first" in texts or "needs no eager call first" in texts, export
            n += 1
    assert n >= 30


def test_variant_zero_is_the_data_the_table_always_had():
    """the salt must not move variant 0: a few cases rebuilt here from numpy's generator alone"""
    ctx = _dry_ctx()

    def plain(*key):
        return np.random.default_rng(zlib.crc32(repr(key).encode()))

    def U(r, *shape, dtype=np.float32):
        return r.uniform(-1.0, 1.0, shape).astype(dtype)

    (c,) = [c for c in A.TABLE["gnnmp_add_f32"](ctx) if c.sid == "n128"]
    r = plain("add", 128)
    assert np.array_equal(c.arrs[0].data, U(r, 128)) and np.array_equal(c.arrs[1].data, U(r, 128))

    (c,) = [c for c in A.TABLE["gnnmp_gather_f64"](ctx) if c.sid == "K33_D1_i8b1"]
    r = plain("gnnmp_gather_f64", 33, 1, 8, 1)
    assert np.array_equal(c.arrs[0].data, U(r, 50, 1, dtype=np.float64)) and np.array_equal(c.arrs[1].data, r.integers(1, 51, 33))

    (c,) = [c for c in A.TABLE["gnnmp_propagate_f32"](ctx) if c.sid.startswith("hub_D2_")]
    g = ctx.hub
    r = plain("gnnmp_propagate_f32", "hub", 2)
    want = {"xj": U(r, g.n_src, 2), "w": U(r, g.E), "scale_src": (0.5 + r.random(g.n_src)).astype(np.float32),
            "scale_dst": (0.5 + r.random(g.n_dst)).astype(np.float32)}
    assert {a.name for a in c.arrs if a.role == "in"} == set(want)
    for a in c.arrs:
        if a.role == "in":
            assert np.array_equal(a.data, want[a.name]), a.name

    (c,) = [c for c in A.TABLE["gnnmp_inv_sqrt_f32"](ctx) if c.sid == "n33"]
    assert np.array_equal(c.arrs[0].data, (1.0 + plain("inv_sqrt", 33).integers(0, 50, 33)).astype(np.float32))


def _same_call(c0, c1):
    """problems if two variants of a case are not the same call on other float data; the names of the float inputs that differ"""
    problems, differ, floats = [], [], 0
    args0, args1 = list(A.flat_args(c0.args)), list(A.flat_args(c1.args))          # records opened: their fields are arguments like any other
    if (c0.sid, c0.status, c0.knobs, len(args0), c0.no_warmup) != (c1.sid, c1.status, c1.knobs, len(args1), c1.no_warmup):
        return [f"{c0.export}[{c0.sid}] is another call in the other variant"], differ, floats
    seen = set()
    for a0, a1 in zip(args0, args1):
        if isinstance(a0, A.Arr) and a0.base is not None:
            if not (isinstance(a1, A.Arr) and a1.base is not None and (a0.name, a0.role, a0.base.name, a0.offset) == (a1.name, a1.role, a1.base.name, a1.offset)):
                problems.append(f"view '{a0.name}' is another view")
                continue
            a0, a1 = a0.base, a1.base                # the bytes are the base's: compared once, under its name
        if isinstance(a0, A.Arr):
            if a0.name in seen:
                continue
            seen.add(a0.name)
            if not isinstance(a1, A.Arr) or (a0.name, a0.role, a0.shape, a0.dtype) != (a1.name, a1.role, a1.shape, a1.dtype):
                problems.append(f"array '{a0.name}' has another role, shape or type")
            elif a0.data is not None:
                same = np.array_equal(a0.data, a1.data, equal_nan=a0.dtype.kind == "f")
                if a0.dtype.kind == "f":
                    floats += a0.data.size > 0
                    if not same:
                        differ.append(a0.name)
                elif not same:
                    problems.append(f"index array '{a0.name}' differs between the variants")
        elif isinstance(a0, A.Pl):
            if not (isinstance(a1, A.Pl) and (a0.T, a0.loops) == (a1.T, a1.loops) and np.array_equal(a0.g.s, a1.g.s)
                    and np.array_equal(a0.g.t, a1.g.t) and (a0.g.n_src, a0.g.n_dst) == (a1.g.n_src, a1.g.n_dst)):
                problems.append("the plan is of another graph")
        elif a0 is A.STREAM or isinstance(a0, A.HostOut):
            if type(a0) is not type(a1):
                problems.append("argument kinds differ")
        elif a0 != a1:
            problems.append(f"scalar argument {a0!r} != {a1!r}")
    return problems, differ, floats


def test_the_variants_are_the_same_calls_on_other_float_inputs():
    ctx0, ctx1 = _dry_ctx(0), _dry_ctx(1)
    n = 0
    for export in A.capturable():
        cs0, cs1 = _capture_cases(ctx0, export), _capture_cases(ctx1, export)
        assert len(cs0) == len(cs1) >= 1 and sum("side" in c.tags for c in cs0) == 1, export
        if _takes_plan(export):
            assert any("ws" in c.tags for c in cs0), export
        for c0, c1 in zip(cs0, cs1):
            problems, differ, floats = _same_call(c0, c1)
            assert not problems, (export, c0.sid, problems)
            assert bool(differ) == bool(floats), f"{export}[{c0.sid}]: the float inputs of the two variants do not differ"
            n += 1
    assert n > 80


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU: the capture helper
# ------------------------------------------------------------------------------------------------------------------------------------
_BROKEN = None      # set when a capture could not be ENDED: the stream / the allocator may be left recording, nothing more is started


def _require_working_capture():
    if _BROKEN is not None:
        pytest.fail(f"an earlier capture of this file could not be ended ({_BROKEN}): no further GPU work is started here")


def capture(fn, stream):
    """record fn() on `stream` into a graph: (graph, what fn returned, problems met — empty if the capture went through).  A host wait
    or an allocation by the calling thread is an error (thread_local), the capture is ended in any case and the device synchronised;
    nothing is retried"""
    global _BROKEN
    import torch
    _require_working_capture()
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    out, err = None, []
    with torch.cuda.stream(stream):
        graph.capture_begin(capture_error_mode="thread_local")
        try:
            out = fn()
        except Exception as e:           # reported below, after the capture has been ended
            err.append(f"the call raised {type(e).__name__}: {e}")
        finally:
            try:
                graph.capture_end()
            except Exception as e:
                _BROKEN = f"{type(e).__name__}: {e}"
                err.append(f"ending the capture raised {_BROKEN}")
            try:
                torch.cuda.synchronize()
            except Exception as e:
                _BROKEN = f"{type(e).__name__}: {e}"
                err.append(f"the synchronisation after the capture raised {_BROKEN}")
    return graph, out, err


@pytest.fixture(scope="module")
def lib():
    import torch
    assert torch.cuda.is_available()
    from gnnmp import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def ctxs(lib):
    thr = A.plan_threshold(lib, _dry_ctx().hub.E)          # the threshold a plan of the hub graph's size gets: read, not assumed
    return A.Ctx(thr, variant=0), A.Ctx(thr, variant=1)


@pytest.fixture(scope="module")
def side():
    import torch
    return torch.cuda.Stream()


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU: every capturable export, recorded and replayed
# ------------------------------------------------------------------------------------------------------------------------------------
def _same_bits(got, want, what):
    return [f"output '{n}' of {what}" for n in want if not np.array_equal(got[n], want[n])]


def _record_and_replay(lib, c0, c1, plans, side):
    import torch
    problems, differ, _ = _same_call(c0, c1)
    if problems:
        return problems
    slab = A.Slab(c0.arrs, "cuda", None, c0.guard)
    cargs, host = A.bind(c0, slab, plans, side)
    assert not host, "an export that hands a result to the host cannot be launch-only"
    torch.cuda.synchronize()

    # 1. eager, on the capture stream: the documented first-use growth of plan scratch and the one-time LDS opt-in happen here.  An
    # export whose comment says it "may be recorded into a HIP graph without an eager call first" is recorded cold: its plans are new
    # (this test's own), nothing has run on them, and the eager bits are taken AFTER the replays instead
    eager = None
    if not c0.no_warmup:
        rc = A.call(lib, c0, cargs)
        torch.cuda.synchronize()
        problems = A.verify(c0, rc, slab, {})
        if problems:
            return ["eager warm-up: " + p for p in problems]
        eager = slab.outputs()
        slab.reload()

    # 2. capture: the call is recorded, nothing runs
    graph, rc, err = capture(lambda: A.call(lib, c0, cargs), side)
    if err or rc != c0.status:
        return [f"under stream capture the call returned {rc} (expected {c0.status}); gnnmp_last_error: "
                f"{lib.gnnmp_last_error().decode(errors='replace')!r}"] + err
    problems = slab.check({}, untouched=True)
    if problems:
        return ["while the call was being recorded (work ran at capture time, or went to another stream): " + p for p in problems]
    if rc != A.OK:
        return []                                  # a refusal records nothing: there is nothing to replay

    # 3. replay 1: the eager bits
    graph.replay()
    torch.cuda.synchronize()
    problems = ["replay 1: " + p for p in A.verify(c0, rc, slab, {})]
    if eager is None and not problems:
        first = slab.outputs()
        slab.reload()
        assert A.call(lib, c0, cargs) == rc
        torch.cuda.synchronize()
        eager = slab.outputs()
        slab.reload()
        graph.replay()
        torch.cuda.synchronize()
        problems += [p + " differs between the cold replay and the one after an eager call" for p in _same_bits(slab.outputs(), first, "replay 1")]
    if "_atomic_" not in c0.export:      # (the header's determinism rule leaves *_atomic_* out: A.verify's bound above is what it owes)
        problems += [p + " differs between the eager call and replay 1" for p in _same_bits(slab.outputs(), eager, "replay 1")]
    if problems:
        return problems

    # 4. new values at the same addresses
    slab.reload({a.name: a.data for a in c1.arrs if a.name in differ})
    graph.replay()
    torch.cuda.synchronize()
    problems = ["replay 2, new values in the same buffers: " + p for p in A.verify(c1, rc, slab, {})]
    if problems:
        return problems
    second = slab.outputs()

    # 5. back to back: no host synchronisation, no re-poisoning between the two
    if any(a.role == "inout" for a in c0.arrs):
        # an in-out array (an accumulator the caller pre-fills, a buffer updated in place) carries the first launch's result into the
        # second, so the bits of ONE launch are not owed: the same two launches made eagerly are the reference.  *_atomic_* is the one
        # family the header's determinism rule leaves out (order of the float adds undefined): the table's bound instead of the bits
        slab.reload()
        for _ in range(2):
            assert A.call(lib, c0, cargs) == rc
        torch.cuda.synchronize()
        want = slab.outputs()
        slab.reload()
        graph.replay()
        graph.replay()
        torch.cuda.synchronize()
        got = slab.outputs()
        del graph
        if "_atomic_" not in c0.export:
            return [p + " differs from the same two calls made eagerly" for p in _same_bits(got, want, "two replays back to back")]
        problems = []
        for a in c0.arrs:
            if a.role == "inout":
                g64, w64 = got[a.name].view(a.dtype).astype(np.float64), want[a.name].view(a.dtype).astype(np.float64)
                if np.abs(g64 - w64).max() > A.RTOL * max(np.abs(w64).max(), 1e-30):
                    problems.append(f"output '{a.name}' of two replays back to back is not within {A.RTOL:g} of the same two calls made eagerly")
        return problems
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    problems = [] if "_atomic_" in c0.export else \
        [p + " differs from replay 2" for p in _same_bits(slab.outputs(), second, "replays 3 and 4, back to back,")]
    problems += ["replays 3 and 4: " + p for p in A.verify(c1, rc, slab, {})]
    del graph
    return problems


@gpu
@pytest.mark.parametrize("export", A.capturable())
def test_capture_replay_new_values_and_back_to_back(lib, ctxs, side, export):
    _require_working_capture()
    plans = A.Plans(lib)
    failures = []
    try:
        for c0, c1 in zip(_capture_cases(ctxs[0], export), _capture_cases(ctxs[1], export)):
            _require_working_capture()
            problems = _record_and_replay(lib, c0, c1, plans, side)
            if problems:
                failures.append(f"{export}[{c0.sid}]:\n  " + "\n  ".join(problems))
    finally:
        plans.close()
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU: whole steps of the Python mirror as one graph
# ------------------------------------------------------------------------------------------------------------------------------------
def hub_graph_np(n=300, E=1500, hub=700, seed=3):
    """1-based (s, t): a destination and a source of `hub` edges each (above GNNMP_LONG_ROW: split in the plan and in the transposed
    plan), five isolated nodes at the end, every tenth edge doubled (multi-edges), no self loops"""
    rng = np.random.default_rng(seed)
    m = n - 5
    s, t = rng.integers(0, m, E), rng.integers(0, m, E)
    s = np.concatenate([s, rng.integers(0, m, hub), np.full(hub, 11), s[::10]])
    t = np.concatenate([t, np.full(hub, 7), rng.integers(0, m, hub), t[::10]])
    keep = s != t
    p = rng.permutation(int(keep.sum()))
    return s[keep][p] + 1, t[keep][p] + 1, n


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _graph(gm, s, t, n):
    g = gm.GNNGraph(_dev(s), _dev(t), num_nodes=n)
    for plan in (g.plan(False), g.plan(True)):
        assert plan.n_long >= 1, "the graph of the layer steps must have a split row"
    return g


def _same_tensor_bits(a, b):
    import torch
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _step_as_graph(side, inputs, fresh, step, check, then=None):
    """inputs: {name: static tensor}; fresh: {name: numpy values to copy in after the capture}; step() -> tuple of float32 tensors
    (outputs and gradients); check(tuple of numpy arrays): the reference's bars on the fresh values; then: values for one more round
    after the back-to-back replays (replayed once, compared with the eager step).  Equality is of the bits (NaNs included)"""
    import torch
    _require_working_capture()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):                       # plans, norm caches, workspaces: built before the capture
            step()
    torch.cuda.synchronize()
    graph, outs, err = capture(step, side)
    assert not err, "the step cannot be recorded: " + "; ".join(err)
    with torch.no_grad():
        for name, v in fresh.items():
            inputs[name].copy_(_dev(v))
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    got = [o.clone() for o in outs]
    with torch.cuda.stream(side):
        eager = step()
    torch.cuda.synchronize()
    for k, (a, b) in enumerate(zip(got, eager)):
        assert _same_tensor_bits(a, b), f"output {k} of the replay on fresh values differs from the eager step on the same values"
    check([o.cpu().numpy() for o in got])
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    for k, (a, b) in enumerate(zip(outs, got)):
        assert _same_tensor_bits(a, b), f"output {k} of two replays back to back differs from the single replay"
    if then is not None:
        with torch.no_grad():
            for name, v in then.items():
                inputs[name].copy_(_dev(v))
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        last = [o.clone() for o in outs]
        with torch.cuda.stream(side):
            eager = step()
        torch.cuda.synchronize()
        for k, (a, b) in enumerate(zip(last, eager)):
            assert _same_tensor_bits(a, b), f"output {k} of a replay after the back-to-back replays differs from the eager step"
        return last


@pytest.fixture(scope="module")
def gm():
    import torch
    assert torch.cuda.is_available()
    import gnnmp
    gnnmp.load()
    return gnnmp


@gpu
def test_gcn_and_gat_forward_step(gm, oracle, side):
    """the bench step scaled down: GCNConv(relu) and GATConv(8 heads, relu) on one graph"""
    from test_tgcn import close
    s, t, n = hub_graph_np()
    D = 64
    rng = np.random.default_rng(1)
    x0, x1 = (rng.standard_normal((n, D)).astype(np.float32) for _ in range(2))
    g = _graph(gm, s, t, n)
    gcn = gm.GCNConv((D, D), "relu", seed=1)
    gat = gm.GATConv((D, 8), "relu", heads=8, seed=2)
    x = _dev(x0)

    def check(got):
        close(got[0], oracle.gcn_conv(s, t, n, x1, gcn.weight.cpu().numpy(), gcn.bias.cpu().numpy(), "relu"), "GCNConv")
        close(got[1], oracle.gat_conv(s, t, n, x1, gat.dense_x_weight.cpu().numpy(), gat.a.cpu().numpy(), gat.bias.cpu().numpy(),
                                      "relu", heads=8), "GATConv")
    _step_as_graph(side, {"x": x}, {"x": x1}, lambda: (gcn(g, x), gat(g, x)), check)


def _chain_batch(gm, rng):
    """a batch for the wave-pair chain kernel (members of at most 64 nodes) with a split row: one member's node collects 200 edges"""
    from test_graph_chain import build, random_members
    from gnnmp import _lib, layers
    members = random_members(40, rng, nmin=1, nmax=60)
    k = int(rng.integers(0, 64, 1)[0])
    members.append((np.concatenate([rng.integers(1, 65, 200), [3, 3, 3]]), np.concatenate([np.full(200, 1 + k % 60), [5, 5, 5]]), 64))
    xs = [rng.standard_normal((m[2], 16), dtype=np.float32) for m in members]
    g = gm.batch_arrays(members, xs)
    assert g.plan(False).n_long >= 1, "the batch must have a split row"
    model = build(gm, (16, 128, 128), 2, "+", "mean")
    assert layers._chain_pattern(model.layers) is not None
    # the step must be the fused chain, not the layer-by-layer fallback: the one C call returns GNNMP_OK (tests/test_graph_chain.py:
    # test_fused_kernel_is_taken) and the batch has wave jobs, so csrc/graph_chain2.hip's kernel pair runs it
    lib = _lib.load()
    real, calls = lib.gnnmp_graphconv_chain_f32, []

    class Spy:
        def __call__(self, *a):
            calls.append(real(*a))
            return calls[-1]
    try:
        lib.gnnmp_graphconv_chain_f32 = Spy()
        model(g, g.x)
    finally:
        lib.gnnmp_graphconv_chain_f32 = real
    assert calls == [0], calls
    assert g._cache["chain_jobs"].njobs > 0 and gm.knob(gm.Knob.CHAIN) == 0
    return members, xs, g, model


@gpu
def test_config5_chain_forward_step(gm, oracle, side):
    """GNNChain(GraphConv(16 => 128, relu), GraphConv(128 => 128, relu), GlobalPool(mean), Dense(128 => 2)) on a batch, as bench.py
    runs it: the fused chain kernel with its job tables"""
    from test_graph_chain import close, oracle_chain
    rng = np.random.default_rng(5)
    members, xs0, g, model = _chain_batch(gm, rng)
    xs1 = [rng.standard_normal((m[2], 16), dtype=np.float32) for m in members]

    def check(got):
        close(got[0], oracle_chain(oracle, members, xs1, model.layers[:2], "mean", model.layers[-1]), "the fused GraphConv chain")
    _step_as_graph(side, {"x": g.x}, {"x": np.concatenate(xs1)}, lambda: (model(g, g.x),), check)


@gpu
def test_config5_chain_replayed_on_non_finite_features(gm, oracle, side):
    """the chain kernel's set-aside list: recorded on finite features, replayed on features with Inf / NaN in three member graphs (their
    tiles are set aside and redone in fp32 loops), three times, then once more on finite features.  The counter of set-aside jobs must
    be back at zero after every launch: a counter that only the NEXT host call re-arms grows from replay to replay"""
    import torch
    from test_graph_chain import close, oracle_chain
    rng = np.random.default_rng(6)
    members, xs0, g, model = _chain_batch(gm, rng)
    xs1 = [rng.standard_normal((m[2], 16), dtype=np.float32) for m in members]
    hit = [3, 17, len(members) - 1]                       # the last one is the member with the split row
    assert all(members[k][2] >= 2 for k in hit)
    xs1[hit[0]][1, 2] = np.inf
    xs1[hit[1]][0, 0] = np.nan
    xs1[hit[2]][1] = -np.inf
    xs2 = [rng.standard_normal((m[2], 16), dtype=np.float32) for m in members]
    # the bits of the step on the last round's finite values, taken BEFORE any job was ever set aside: an eager call made after the
    # replays would share whatever state they left behind, and agree with them
    with torch.no_grad():
        g.x.copy_(_dev(np.concatenate(xs2)))
        clean = model(g, g.x).clone()
        g.x.copy_(_dev(np.concatenate(xs0)))
    torch.cuda.synchronize()

    def check(got):
        y = got[0]
        with gm.tuned(gm.Knob.CHAIN, -1):                                   # the layer-by-layer path on the same values (tests/test_graph_chain.py: run_both)
            yl = model(g, g.x).cpu().numpy()
        bad = np.flatnonzero(~np.isfinite(y).all(1)).tolist()
        assert bad == np.flatnonzero(~np.isfinite(yl).all(1)).tolist() == sorted(hit), bad
        assert np.array_equal(np.isnan(y), np.isnan(yl))
        good = np.isfinite(y).all(1)
        ref = oracle_chain(oracle, members, xs1, model.layers[:2], "mean", model.layers[-1])
        close(y[good], ref[good], "the member graphs with finite features")
    last = _step_as_graph(side, {"x": g.x}, {"x": np.concatenate(xs1)}, lambda: (model(g, g.x),), check, then={"x": np.concatenate(xs2)})
    assert _same_tensor_bits(last[0], clean), "after replays that set jobs aside, a replay on finite features redoes stale jobs"
    y = model(g, g.x)
    torch.cuda.synchronize()
    close(y.cpu().numpy(), oracle_chain(oracle, members, xs2, model.layers[:2], "mean", model.layers[-1]), "finite features again")


@gpu
def test_gcn_and_gat_training_step(gm, oracle, side):
    """forward and backward of a GCN and a GAT layer through gnnmp.backward"""
    import torch
    from gnnmp.backward import gat_conv_ad, gcn_conv_ad
    from test_tgcn import close
    s, t, n = hub_graph_np()
    Din, Dout, H, C = 24, 24, 4, 8
    rng = np.random.default_rng(2)
    x0, x1 = (rng.standard_normal((n, Din)).astype(np.float32) for _ in range(2))
    r0, r1 = (rng.standard_normal((n, Dout)).astype(np.float32) for _ in range(2))
    q0, q1 = (rng.standard_normal((n, H * C)).astype(np.float32) for _ in range(2))
    g = _graph(gm, s, t, n)
    gcn = gm.GCNConv((Din, Dout), "relu", seed=5)
    gcn.bias = _dev(rng.standard_normal(Dout).astype(np.float32) * 0.1)
    gat = gm.GATConv((Din, C), "relu", heads=H, seed=3)
    gat.bias = _dev((rng.standard_normal(H * C) * 0.1).astype(np.float32))
    params = [gcn.weight, gcn.bias, gat.dense_x_weight, gat.a, gat.bias]
    for p in params:
        p.requires_grad_(True)
    x, r, q = _dev(x0).requires_grad_(True), _dev(r0), _dev(q0)

    def step():
        y1, y2 = gcn_conv_ad(gcn, g, x), gat_conv_ad(gat, g, x)
        g1 = torch.autograd.grad(y1, [x, gcn.weight, gcn.bias], r)
        g2 = torch.autograd.grad(y2, [x, gat.dense_x_weight, gat.a, gat.bias], q)
        return (y1.detach(), y2.detach()) + tuple(g1) + tuple(g2)

    def check(got):
        W, b = gcn.weight.detach().cpu().numpy(), gcn.bias.detach().cpu().numpy()
        Wx, a, ba = (p.detach().cpu().numpy() for p in (gat.dense_x_weight, gat.a, gat.bias))
        close(got[0], oracle.gcn_conv(s, t, n, x1, W, b, "relu"), "GCNConv")
        close(got[1], oracle.gat_conv(s, t, n, x1, Wx, a, ba, "relu", heads=H), "GATConv")
        for nm, a_, b_ in zip(("dx", "dW", "db"), got[2:5], oracle.grad_gcn_conv(s, t, n, x1, W, b, "relu", r1)):
            close(a_, b_, "GCNConv " + nm)
        for nm, a_, b_ in zip(("dx", "dW", "da", "db"), got[5:9], oracle.grad_gat_conv(s, t, n, x1, Wx, a, ba, "relu", q1, heads=H)):
            close(a_, b_, "GATConv " + nm)
    _step_as_graph(side, {"x": x, "r": r, "q": q}, {"x": x1, "r": r1, "q": q1}, step, check)


@gpu
def test_tgcn_training_step(gm, side):
    """TGCN forward and backward, the recurrence in one launch"""
    import torch
    from gnnmp import layers_temporal
    from test_tgcn import close, ref_gcn, ref_tgcn
    s, t, n = hub_graph_np()
    cin, cout, T = 3, 16, 3
    assert layers_temporal.use_fused(cout)
    rng = np.random.default_rng(9)
    x0, x1 = (rng.standard_normal((n, T, cin)).astype(np.float32) for _ in range(2))
    d0, d1 = (rng.standard_normal((n, T, cout)).astype(np.float32) for _ in range(2))
    g = _graph(gm, s, t, n)
    layer = gm.TGCN((cin, cout), seed=0)
    params = [p for p in layer.cell.parameters() if p is not None]
    for p in params:
        p.requires_grad_()
    x, dy = _dev(x0).requires_grad_(), _dev(d0)

    def step():
        y = gm.tgcn_ad(layer, g, x)
        return (y.detach(),) + tuple(torch.autograd.grad(y, [x] + params, dy))

    def check(got):
        ps = [None if p is None else p.detach().cpu().double().requires_grad_() for p in layer.cell.parameters()]
        xr = torch.from_numpy(x1).double().requires_grad_()
        s0, t0 = torch.from_numpy(s - 1), torch.from_numpy(t - 1)
        # a condition on the INPUTS: the gradient of relu jumps at 0, so a float64 reference says nothing about a float32 gradient
        # where a layer-1 pre-activation lies within float32 rounding of 0 (here: a sum of up to 700 terms of size <= 1, rounding
        # ~1e-6).  Every pre-activation of the reference must be 1e-5 or more away from it (one draw in a few is not: seed 4 has
        # one at 1.8e-8, and plain float32 torch then misses the float64 gradient by 7e-3)
        with torch.no_grad():
            pre = [ref_gcn(s0, t0, n, xr[:, k], ps[6 * c], ps[6 * c + 1], False, True).abs().min() for k in range(T) for c in range(3)]
        assert min(float(v) for v in pre) > 1e-5, "the inputs put a relu of layer 1 on its kink: pick other inputs"
        ref = ref_tgcn(s0, t0, n, xr, ps)
        ref_g = torch.autograd.grad(ref, [xr] + [p for p in ps if p is not None], torch.from_numpy(d1).double())
        close(got[0], ref, "TGCN forward")
        for k, (a, b) in enumerate(zip(got[1:], ref_g)):
            close(a, b, f"TGCN gradient {k}")
    _step_as_graph(side, {"x": x, "dy": dy}, {"x": x1, "dy": d1}, step, check)


@gpu
def test_dot_decoder_training_step(gm, side):
    import torch
    from test_linkpred import _close, _np_grads
    s, t, n = hub_graph_np()
    D = 33
    rng = np.random.default_rng(8)
    x0, x1 = (rng.standard_normal((n, D)).astype(np.float32) for _ in range(2))
    d0, d1 = (rng.standard_normal(len(s)).astype(np.float32) for _ in range(2))
    g = _graph(gm, s, t, n)
    x, dz = _dev(x0).requires_grad_(True), _dev(d0)

    def step():
        z = gm.dot_decoder_ad(g, x)
        return (z.detach(),) + tuple(torch.autograd.grad(z, [x], dz[:, None]))

    def check(got):
        _close(got[0], np.sum(x1[t - 1].astype(np.float64) * x1[s - 1], axis=1, keepdims=True))
        _close(got[1], sum(_np_grads(s, t, x1, x1, d1)))
    _step_as_graph(side, {"x": x, "dz": dz}, {"x": x1, "dz": d1}, step, check)
