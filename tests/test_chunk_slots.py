"""Knob.CHUNK_SLOTS (csrc/knobs.h, csrc/plan.hip: plan_chunk_slots): the chunk length of split rows is read at plan build.  The smallest
plan that splits: about 300 nodes and one destination of 1 500 in-edges with the long-row threshold forced down to 64, so the hub's
chunks are 16 slots long under the knob and min(64, 128) = 64 slots long at its default.  Reference semantics of the rows themselves:
GNNlib/src/msgpass.jl:71-79 (propagate)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CHUNK_TABLE_BYTES = 16      # per chunk: chunk_row, chunk_lrow (int32), chunk_beg, chunk_end (uint32): csrc/plan.hip plan_build_long_rows


def test_chunk_slots_knob_sets_the_chunk_length_at_plan_build(oracle):
    import torch
    import gnnmp as gm
    import test_gpu_parity as T
    from test_fold_stress import hub_graph
    gm.load()
    rng = np.random.default_rng(23)
    n, D = 300, 8
    s, t = hub_graph(rng, n, 3000, [(17, 1500)])
    x = rng.standard_normal((n, D)).astype(np.float32)
    xd = torch.from_numpy(x).cuda()

    def build(slots):
        with gm.tuned(gm.Knob.LONG_ROW, 64), gm.tuned(gm.Knob.CHUNK_SLOTS, slots):
            g = gm.GNNGraph(torch.from_numpy(s).cuda(), torch.from_numpy(t).cuda(), num_nodes=n)      # (the constructor builds the plan)
            return g, g.plan(False)

    g16, p16 = build(16)
    g0, p0 = build(0)
    assert gm.knob(gm.Knob.CHUNK_SLOTS) == 0 and gm.knob(gm.Knob.LONG_ROW) == 0
    hub = p0.max_degree
    assert p16.long_thresh == p0.long_thresh == 64 and p16.n_long == p0.n_long == 1 and 1500 <= hub == p16.max_degree
    # gnnmp_plan_info reports the device bytes a fresh plan holds; the two plans differ by their chunk tables alone
    chunks16, chunks64 = -(-hub // 16), -(-hub // 64)
    print(f"hub of {hub} slots: {chunks16} against {chunks64} chunks predicted, plan bytes {p16.bytes} against {p0.bytes}")
    assert p16.bytes - p0.bytes == CHUNK_TABLE_BYTES * (chunks16 - chunks64)

    m16 = gm.propagate(gm.copy_xj, g16, "max", xj=xd)
    m0 = gm.propagate(gm.copy_xj, g0, "max", xj=xd)
    assert torch.equal(m16.view(torch.int32), m0.view(torch.int32))
    ref = oracle.propagate("+", s, t, n, x, None, n_dst=n)
    for g in (g16, g0):
        T.assert_close(T.host(gm.propagate(gm.copy_xj, g, "+", xj=xd)), ref)
    assert gm.knob(gm.Knob.CHUNK_SLOTS) == 0
