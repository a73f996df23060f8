"""The cases of the TopKPool exports (csrc/topk.hip, csrc/plan_edit.hip) for the ABI's memory contract, kept beside tests/abi_cases.py
instead of in it: that module is a yardstick and stays as it is.  Importing this module registers
  gnnmp_topk_score_f32, gnnmp_topk_select_f32, gnnmp_topk_gate_f32, gnnmp_topk_gate_grad_f32   in TABLE (they only launch), and
  gnnmp_plan_keep_nodes                                                                        in PREP_TABLE (it synchronises once),
wrapped for the variants as the registry wraps its own builders.  As with tests/ppr_cases.py, the registry knows them in a session
that has imported this module (tests/test_topk_abi.py does, so a run of the whole suite has them when the completeness guard
executes); the parametrised tests of tests/test_abi_memory_contract.py and tests/test_abi_graph_capture.py take their export lists
before that, so tests/test_topk_abi.py runs the same checks over these cases itself.

keep and rank are exact (tests/topk_ref.py); the float outputs owe the table's 1e-5 of the float64 restatement's scale."""
import ctypes

import numpy as np

import abi_cases as A
import topk_ref as R

SCORE, SELECT, GATE, GRAD, KEEP = ("gnnmp_topk_score_f32", "gnnmp_topk_select_f32", "gnnmp_topk_gate_f32", "gnnmp_topk_gate_grad_f32",
                                   "gnnmp_plan_keep_nodes")
LAUNCH_ONLY = (SCORE, SELECT, GATE, GRAD)
CS = (1, 3, 7, 64, 100, 129, 513)               # one lane a row, L below C's power of two, 64 lanes with 2, 3 and 9 strides
DEV_FROM_12 = 4 * 11                            # lds_budget_bytes that holds 11 keys: member graphs of 12 and more take the device route


def _row_shapes():
    """(N, C, tags): every width at 33 rows; one row; 300 rows at a narrow and a wide C"""
    for k, C in enumerate(CS):
        yield 33, C, ({"align", "side"} if k == 2 else {"align"} if C in (3, 64) else set())
    for N, C in ((1, 7), (300, 3), (300, 100)):
        yield N, C, set()


def build_score(ctx):
    for N, C, tags in _row_shapes():
        r = A.rng_of("topk_score", N, C)
        x, p = A.F(r, N, C), A.F(r, C)
        yield A.mk(SCORE, f"N{N}_C{C}", tags, [A.Arr("x", "in", x), A.Arr("p", "in", p), A.Arr("y", "out", shape=(N,)), N, C, A.STREAM],
                   lambda host, x=x, p=p: {"y": A.E(R.score64(x, p), "rel")})


def build_select(ctx):
    ptr = R.batch_ptr()
    N = int(ptr[-1])
    sv = R.score_vectors(ptr)
    # (graph_ptr width | None, N, lds_budget_bytes, k, ratio, ties, scores: a name of R.score_vectors | "F" (the table's own draw), rank?)
    shapes = [(8, N, 0, 4, 0.0, R.FIRST, "F", True, {"align", "side"}), (4, N, DEV_FROM_12, 4, 0.0, R.ALL, "tie_block", True, {"align"}),
              (8, N, DEV_FROM_12, 0, 0.5, R.FIRST, "specials", False, ()), (4, N, 0, 64, 0.0, R.ALL, "equal", True, ()),
              (None, 300, 0, 64, 0.0, R.FIRST, "F", True, {"align"}), (None, 300, DEV_FROM_12, 0, 0.1, R.ALL, "equal", False, ()),
              (None, 1500, 0, 2000, 0.0, R.FIRST, "F", True, ()), (None, 0, 0, 1, 0.0, R.FIRST, "F", True, ()),
              (8, N, 64 * 1024, 0, 1.0, R.FIRST, "descending", True, ())]
    for pb, n, budget, k, ratio, ties, kind, want_rank, tags in shapes:
        r = A.rng_of("topk_select", pb, n, budget, k, ratio, ties, kind)
        score = A.F(r, n) if kind == "F" else sv[kind][:n]
        gp = None if pb is None else ptr.astype(np.int64 if pb == 8 else np.int32)

        def ref(host, v=(score, None if pb is None else ptr, k, ratio, ties), want_rank=want_rank, n=n):
            keep, rank = R.select(*v)
            return {"keep": A.E(keep, "exact"), **({"rank": A.E(rank, "exact")} if want_rank and n else {})}
        job = A.Rec("gnnmp_topk_t", score=A.Arr("score", "in", score) if n else None, graph_ptr=A.Arr("graph_ptr", "in", gp) if pb else None,
                    idx_bytes=pb or 8, n_graphs=len(ptr) - 1 if pb else 1, k=k, ratio=ratio, ties=ties, lds_budget_bytes=budget,
                    keep=A.Arr("keep", "out", shape=(n + 1,), dtype=np.uint32),
                    rank=A.Arr("rank", "out", shape=(n,), dtype=np.int32) if want_rank and n else None)
        yield A.mk(SELECT, f"p{pb or 0}_N{n}_b{budget}_k{k}_r{ratio}_t{ties}_{kind}", tags, [job, n, A.STREAM], ref)


def _kept(r, N):
    """an ascending subset of the N nodes (an integer draw: the same in every variant) and its inverse map"""
    pick = np.sort(r.permutation(N)[: max(1, (2 * N) // 3)]).astype(np.int32)
    new = np.full(N, -1, np.int32)
    new[pick] = np.arange(len(pick), dtype=np.int32)
    return pick, new


def build_gate(ctx):
    for k, (N, C, tags) in enumerate(_row_shapes()):
        r = A.rng_of("topk_gate", N, C)
        x, y = A.F(r, N, C), 2.0 * A.F(r, N)
        pick, _ = _kept(r, N)
        act = k % 3
        job = A.Rec("gnnmp_topk_gate_t", x=A.Arr("x", "in", x), y=A.Arr("y", "in", y), node_map=A.Arr("node_map", "in", pick), act=act,
                    out=A.Arr("out", "out", shape=(len(pick), C)))
        yield A.mk(GATE, f"N{N}_C{C}_act{act}", tags, [job, len(pick), C, A.STREAM],
                   lambda host, v=(x, y, pick, act): {"out": A.E(R.gate64(*v), "rel")})


def grad64(x, y, p, dout, new, act):
    """(dx, dy, dp) of gnnmp_topk_gate_grad_f32 in float64, as include/gnnmp.h states them (p None: an external score, no dp)"""
    x, y, dout = np.asarray(x, np.float64), np.asarray(y, np.float64), np.asarray(dout, np.float64)
    kept = new >= 0
    g = R.act64(act, y)
    dg = g * (1 - g) if act == R.SIGMOID else 1 - g * g if act == R.TANH else np.ones_like(y)
    full = np.zeros_like(x)
    full[kept] = dout[new[kept]]
    dy = np.where(kept, dg * (full * x).sum(1), 0.0)
    dx = full * np.where(kept, g, 0.0)[:, None]
    if p is None:
        return dx, dy, None
    p = np.asarray(p, np.float64)
    norm = np.sqrt((p * p).sum())
    dx = dx + dy[:, None] * p[None, :] / norm
    dp = (dy[:, None] * x).sum(0) / norm - (dy * y).sum() * p / norm ** 2
    return dx, dy, dp


def build_grad(ctx):
    for k, (N, C, tags) in enumerate(_row_shapes()):
        r = A.rng_of("topk_gate_grad", N, C)
        x, y, p = A.F(r, N, C), 2.0 * A.F(r, N), A.F(r, C)
        pick, new = _kept(r, N)
        dout = A.F(r, len(pick), C)
        act = k % 3
        with_p, want_dy, want_dp = k % 4 != 3, k % 2 == 0 or k % 4 == 3, k % 4 != 3 and k % 3 != 1
        nb = -(-N // R.GRAD_ROWS)

        def ref(host, v=(x, y, p if with_p else None, dout, new, act), want_dy=want_dy, want_dp=want_dp):
            dx, dy, dp = grad64(*v)
            return {"dx": A.E(dx, "rel"), **({"dy": A.E(dy, "rel")} if want_dy else {}), **({"dp": A.E(dp, "rel")} if want_dp else {})}
        job = A.Rec("gnnmp_topk_gate_grad_t", x=A.Arr("x", "in", x), y=A.Arr("y", "in", y), p=A.Arr("p", "in", p) if with_p else None,
                    dout=A.Arr("dout", "in", dout), node_new=A.Arr("node_new", "in", new), act=act, dx=A.Arr("dx", "out", shape=(N, C)),
                    dy=A.Arr("dy", "out", shape=(N,)) if want_dy else None, dp=A.Arr("dp", "out", shape=(C,)) if want_dp else None,
                    part=A.Arr("part", "scratch", shape=(nb * (C + 1),)) if want_dp else None)
        yield A.mk(GRAD, f"N{N}_C{C}_act{act}_p{int(with_p)}_dy{int(want_dy)}_dp{int(want_dp)}", tags, [job, N, C, A.STREAM], ref)


def build_keep(ctx):
    """the mask gnnmp_plan_remove_nodes would mark for a list gives its child; then all ones, all zeros, a graph of no node"""
    Rm = A._mod("augment_ref")
    if "topk_empty" not in ctx.cache:
        ctx.cache["topk_empty"] = A.Graph("no_nodes", [], [], 0)
    # (graph, self loops, the mask: "list" | "ones" | "zeros", the optional outputs)
    shapes = ((ctx.r33, False, "list", True, {"align", "side"}), (ctx.r300, True, "list", True, {"align"}), (ctx.hub, False, "list", False, ()),
              (ctx.r31, True, "ones", True, ()), (ctx.r33, False, "zeros", True, ()), (ctx.cache["topk_empty"], False, "ones", True, ()))
    for g, loops, what, maps, tags in shapes:
        s0, t0, N = g.s - 1, g.t - 1, g.n
        if what == "list":
            lst = A.rng_of("remove_nodes", g.name).permutation(N)[: max(1, N // 4)]       # the list of the registry's remove_nodes cases
        else:
            lst = np.arange(N) if what == "zeros" else np.zeros(0, np.int64)
        mask = np.full(N, 7, np.uint32)                                                   # any non-zero word keeps
        mask[lst] = 0
        s2, t2, _, n2, nid, eid = Rm.remove_nodes(s0, t0, None, N, lst, base=0)
        new = np.full(N, -1, np.int64)
        new[nid] = np.arange(n2)
        csr = A.csr_of(s2 + 1, t2 + 1, n2, loops)
        arr = lambda name, n, dt: A.Arr(name, "out", shape=(n,), dtype=dt) if n else None      # noqa: E731  (no element: NULL)
        outs = [arr("node_map_out", n2, np.int32), arr("node_new_out", N, np.int32), arr("edge_map_out", len(s2), np.uint32)] if maps else [None] * 3

        def ref(host, v=(n2, len(s2), nid, new, eid, csr), outs=outs):
            A._totals(host, v[0], v[1])
            vals = {"node_map_out": v[2], "node_new_out": v[3], "edge_map_out": v[4]}
            return {**{a.name: A.E(vals[a.name], "exact") for a in outs if a is not None}, **A._csr_ref(v[5], "new_")}
        yield A.mk(KEEP, f"{g.name}_loops{int(loops)}_{what}_maps{int(maps)}", tags,
                   [A.NewPlan("plan"), A.Pl(g, loops=loops), A.Arr("keep", "in", mask) if N else None] + outs +
                   [A.HostOut("total", ctypes.c_int64 * 2), A.STREAM], ref, then=A._exported(n2, csr))


BUILDERS = {SCORE: build_score, SELECT: build_select, GATE: build_gate, GRAD: build_grad}

for _name, _build in BUILDERS.items():
    if _name not in A.TABLE:
        A.TABLE[_name] = A._of_variant(_build)          # as the registry's last lines wrap every builder it holds
if KEEP not in A.PREP_TABLE:
    A.PREP_TABLE[KEEP] = A._of_variant(build_keep)
