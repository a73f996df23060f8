"""The cases of gnnmp_ppr_diffusion_f32 (csrc/ppr.hip) for the ABI's memory contract, kept beside tests/abi_cases.py instead of in it:
that module is a yardstick and stays as it is.  Importing this module registers the builder in the registry's PREP_TABLE — the set-up
calls that synchronise ("Synchronises the stream (graph prep)" in the export's header comment), which nothing records into a HIP graph —
through the registry's own entry (`prep_cases_of`), wrapped for the variants as the registry wraps its own builders.

What follows from the place: the registry knows the export in a session that has imported this module — tests/test_ppr_abi.py and
tests/test_ppr.py do, so a run of the whole suite has it when the completeness guard of tests/test_abi_memory_contract.py executes —
and not in a session that collects that file alone.  The parametrised contract tests of that file take their export lists when it is
imported, before this module: tests/test_ppr_abi.py therefore runs the same three checks (natural alignment, every shifted pointer,
a side stream) over these cases itself, with the registry's slab, run_case and verify.

The reference is not exact: the bar of tests/ppr_ref.py against the float64 restatement, and the table's 1e-5 of the scale."""
import numpy as np

import abi_cases as A

NAME = "gnnmp_ppr_diffusion_f32"
SCRATCH_FROM_12 = 4 * (11 * 11 + 2 * 11)      # lds_budget_bytes that holds 11 nodes: members of 12 and more take the scratch path


def build(ctx):
    import ppr_ref as P
    if "ppr" not in ctx.cache:
        (bs, bt, bn, _), off, _ = P.batch(False)                       # members of 1 .. 127 nodes and two empty ones
        mk_g = lambda name, g: A.Graph(name, g[0] + 1, g[1] + 1, g[2])   # noqa: E731
        ctx.cache["ppr"] = (A.Graph("ppr_batch", bs + 1, bt + 1, bn), off, mk_g("ppr_65", P.members(False)[6]), mk_g("ppr_300", P.large_graph()))
    gbatch, off, g65, g300 = ctx.cache["ppr"]
    # (graph, graph_ptr width | None, lds_budget_bytes, tags)
    shapes = [(gbatch, 8, 0, {"align", "side"}), (gbatch, 4, SCRATCH_FROM_12, ()), (ctx.e0, None, 0, ()), (ctx.one, None, 0, ()),
              (g65, None, 0, {"align"}), (g65, None, SCRATCH_FROM_12, ()), (g300, None, 0, ()), (gbatch, 8, 160 * 1024, ())]
    for k, (g, pb, budget, tags) in enumerate(shapes):
        r = A.rng_of("ppr", g.name, pb, budget)
        w = (0.55 + 0.45 * A.F(r, g.E)).astype(np.float32)             # [0.1, 1]: the conditioning tests/test_ppr_ref.py checks holds
        with_w = k % 2 == 0 and g.E > 0
        gr = (g.s - 1, g.t - 1, g.n, w if with_w else None)
        r64, lap = P.ref64(*gr, P.ALPHA), P.lapack32(*gr, P.ALPHA)

        def ref(host, r64=r64, lap=lap, has_out=g.E > 0):
            how = lambda got: None if P.within_bar(got, lap, r64) else "%.2f times the reference's own float32 error (bar %d)" % (P.ratio(got, lap, r64), P.K)      # noqa: E731
            return {"out": A.E(r64, "rel", pred=how)} if has_out else {}
        job = A.Rec("gnnmp_ppr_t", w=A.Arr("w", "in", w) if with_w else None,
                    graph_ptr=A.Arr("graph_ptr", "in", off.astype(np.int64 if pb == 8 else np.int32)) if pb else None, idx_bytes=pb or 8,
                    n_graphs=len(off) - 1 if pb else 1, alpha=P.ALPHA, lds_budget_bytes=budget,
                    out=A.Arr("out", "out", shape=(g.E,)) if g.E else None)      # (an array of no element is passed as NULL)
        yield A.mk(NAME, f"{g.name}_w{int(with_w)}_p{pb or 0}_b{budget}", tags, [A.Pl(g, T=True), job, A.STREAM], ref)


if NAME not in A.PREP_TABLE:
    A.prep_cases_of(NAME)(build)
    A.PREP_TABLE[NAME] = A._of_variant(A.PREP_TABLE[NAME])      # as the registry's last lines wrap every builder it holds
