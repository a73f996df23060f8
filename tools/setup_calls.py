"""Every export of the host set-up path (plan builds, graph prep, link prediction, neighbour search, chain jobs) driven ONCE through the C
ABI at tiny shapes: N = 100 nodes, E = 1 000 edges, 64 seed nodes, 32 graphs x 16 points with d = 3.  Two uses:

  * `rocprofv3 --hip-trace --stats -d DIR -- python tools/setup_calls.py` (no counters in that run): the per-function HIP call counts of
    the set-up path — hipMalloc, hipFree, hipStreamSynchronize, hipMemcpy*, hipMemsetAsync, hipLaunchKernel — which a refactor of its
    resource handling must leave as they are (profiles/setup_calls_*.csv);
  * tests/test_setup_error_exits.py imports the `Setup` class for the correct and the failing call of each data-dependent error exit.

Every device array is allocated up front; a call allocates nothing through torch."""
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "graphneuralnetworks.jl_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from gnnmp import _lib  # noqa: E402

N, E, SEEDS, GRAPHS, PER_GRAPH, DIM = 100, 1000, 64, 32, 16, 3
I64 = ctypes.c_int64


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Setup:
    """inputs and outputs of every call, 1-based int64 indices; the `bad_*` twins differ in the one entry that trips the error exit"""

    def __init__(self):
        self.lib = _lib.load()
        self.stream = None                      # the legacy default stream, as torch's current stream is
        rng = np.random.default_rng(11)
        s = rng.integers(1, N + 1, E, dtype=np.int64)
        t = rng.integers(1, N + 1, E, dtype=np.int64)
        self.s, self.t = dev(s), dev(t)
        bad_s = s.copy()
        bad_s[17] = N + 1                       # one out-of-range index
        self.bad_s = dev(bad_s)
        order = np.lexsort((s, t))
        colptr = np.concatenate([[0], np.cumsum(np.bincount(t - 1, minlength=N))]).astype(np.int64) + 1
        self.colptr, self.rowval = dev(colptr), dev(s[order])
        bad_colptr = colptr.copy()
        bad_colptr[40] = bad_colptr[41] + 1     # decreasing
        self.bad_colptr = dev(bad_colptr)
        self.rowptr_o = torch.empty(max(N, GRAPHS * PER_GRAPH) + 1, dtype=torch.int32, device="cuda")
        self.col_o = torch.empty(E + GRAPHS * PER_GRAPH * PER_GRAPH, dtype=torch.int32, device="cuda")
        self.eid_o = torch.empty_like(self.col_o)
        seeds = rng.permutation(N)[:SEEDS].astype(np.int64) + 1
        self.seeds = dev(seeds)
        self.offsets = torch.empty(SEEDS + 1, dtype=torch.int64, device="cuda")
        self.eids = torch.zeros(E, dtype=torch.int64, device="cuda")
        self.sub = [torch.zeros(E, dtype=torch.int64, device="cuda") for _ in range(3)]
        node_map = np.zeros(N, np.int32)
        node_map[seeds - 1] = np.arange(1, SEEDS + 1, dtype=np.int32)
        self.node_map = dev(node_map)
        self.umap = torch.zeros(N, dtype=torch.int32, device="cuda")
        self.ufirst = torch.zeros(N, dtype=torch.int32, device="cuda")
        cand = rng.integers(1, N + 1, SEEDS, dtype=np.int64)
        self.cand = dev(cand)
        bad_cand = cand.copy()
        bad_cand[5] = N + 1
        self.bad_cand = dev(bad_cand)
        self.ulist = torch.zeros(SEEDS, dtype=torch.int64, device="cuda")
        self.points = dev(rng.standard_normal((GRAPHS * PER_GRAPH, DIM)).astype(np.float32))
        self.gi = dev(np.repeat(np.arange(1, GRAPHS + 1, dtype=np.int64), PER_GRAPH))
        self.neg = [torch.zeros(2 * E, dtype=torch.int64, device="cuda") for _ in range(2)]
        self.split = [torch.zeros(E, dtype=torch.int64, device="cuda") for _ in range(4)]
        self.sorted_o = [torch.zeros(E, dtype=torch.int64, device="cuda") for _ in range(2)]
        self.seg_ptr = dev(np.arange(0, GRAPHS * PER_GRAPH + 1, PER_GRAPH, dtype=np.int64))
        self.plan = self._new_plan(self.s)[1]
        torch.cuda.synchronize()

    # ---- plans -----------------------------------------------------------------------------------------------------------------------------
    def _new_plan(self, s, validate=1):
        h = ctypes.c_void_p()
        rc = self.lib.gnnmp_plan_create(ctypes.byref(h), _lib.ptr(s), _lib.ptr(self.t), 8, 1, N, N, E, 0, validate, self.stream)
        return rc, h

    def _plan_bytes(self, rc, h):
        """(status, exported arrays) of a freshly built plan; the plan is destroyed"""
        if rc != 0:
            assert h.value is None, "a refused build hands out no plan"
            return rc, None
        info = (I64 * 8)()
        _lib.check(self.lib.gnnmp_plan_info(h, info))
        nd, ne = int(info[1]), int(info[3])
        _lib.check(self.lib.gnnmp_plan_export(h, _lib.ptr(self.rowptr_o), _lib.ptr(self.col_o), _lib.ptr(self.eid_o), self.stream))
        torch.cuda.synchronize()
        out = (self.rowptr_o[:nd + 1].cpu().numpy().copy(), self.col_o[:ne].cpu().numpy().copy(), self.eid_o[:ne].cpu().numpy().copy())
        _lib.check(self.lib.gnnmp_plan_destroy(h))
        return rc, out

    def plan_create(self, bad=False):
        return self._plan_bytes(*self._new_plan(self.bad_s if bad else self.s))

    def plan_from_csc(self, bad=False):
        h = ctypes.c_void_p()
        rc = self.lib.gnnmp_plan_from_csc(ctypes.byref(h), _lib.ptr(self.bad_colptr if bad else self.colptr), _lib.ptr(self.rowval), 8, 1, N,
                                          N, E, 1, self.stream)
        return self._plan_bytes(rc, h)

    def knn_graph(self, bad=False):
        h = ctypes.c_void_p()
        k = PER_GRAPH if bad else 4             # without self loops a graph of 16 points has 15 neighbours to offer
        rc = self.lib.gnnmp_knn_graph_f32(ctypes.byref(h), _lib.ptr(self.points), GRAPHS * PER_GRAPH, DIM, k, _lib.ptr(self.gi), 8, 1, GRAPHS,
                                          0, self.stream)
        return self._plan_bytes(rc, h)

    def radius_graph(self):
        h = ctypes.c_void_p()
        rc = self.lib.gnnmp_radius_graph_f32(ctypes.byref(h), _lib.ptr(self.points), GRAPHS * PER_GRAPH, DIM, ctypes.c_float(1.5),
                                             _lib.ptr(self.gi), 8, 1, GRAPHS, 0, self.stream)
        return self._plan_bytes(rc, h)

    # ---- mini-batch prep -------------------------------------------------------------------------------------------------------------------
    def sample_neighbors(self, bad=False):
        tot = I64(0)
        args = (self.plan, _lib.ptr(self.seeds), 8, 1, SEEDS, 5, 0, 1234, _lib.ptr(self.offsets), _lib.ptr(self.eids))
        if bad:
            _lib.check(self.lib.gnnmp_sample_neighbors(*args, E, ctypes.byref(tot), self.stream))
            return self.lib.gnnmp_sample_neighbors(*args, tot.value - 1, ctypes.byref(tot), self.stream), None   # capacity one short
        rc = self.lib.gnnmp_sample_neighbors(*args, E, ctypes.byref(tot), self.stream)
        torch.cuda.synchronize()
        return rc, (self.offsets.cpu().numpy().copy(), self.eids[:tot.value].cpu().numpy().copy())

    def induced_subgraph(self, bad=False):
        tot = I64(0)
        args = (self.plan, _lib.ptr(self.node_map), _lib.ptr(self.seeds), 8, 1, SEEDS, _lib.ptr(self.offsets))
        outs = tuple(_lib.ptr(x) for x in self.sub)
        if bad:
            _lib.check(self.lib.gnnmp_induced_subgraph(*args, None, None, None, 0, ctypes.byref(tot), self.stream))   # count-only
            return self.lib.gnnmp_induced_subgraph(*args, *outs, tot.value - 1, ctypes.byref(tot), self.stream), None
        rc = self.lib.gnnmp_induced_subgraph(*args, *outs, E, ctypes.byref(tot), self.stream)
        torch.cuda.synchronize()
        return rc, (self.offsets.cpu().numpy().copy(),) + tuple(x[:tot.value].cpu().numpy().copy() for x in self.sub)

    def unique_append(self, bad=False):
        n_new = I64(0)
        self.umap.zero_()                       # in-out: every call starts from the empty set
        rc = self.lib.gnnmp_unique_append(_lib.ptr(self.umap), _lib.ptr(self.ufirst), N, _lib.ptr(self.bad_cand if bad else self.cand), 8, 1,
                                          SEEDS, 0, _lib.ptr(self.ulist), ctypes.byref(n_new), self.stream)
        if bad:
            return rc, None
        torch.cuda.synchronize()
        return rc, (self.umap.cpu().numpy().copy(), self.ulist[:n_new.value].cpu().numpy().copy())

    # ---- the remaining touched exports: correct calls only ----------------------------------------------------------------------------------
    def others(self):
        lib, st, res, tot = self.lib, self.stream, ctypes.c_int(0), I64(0)
        s, t = _lib.ptr(self.s), _lib.ptr(self.t)
        _lib.check(lib.gnnmp_sort_edge_index(s, t, 8, 1, E, _lib.ptr(self.sorted_o[0]), _lib.ptr(self.sorted_o[1]), st))
        _lib.check(lib.gnnmp_is_bidirected(s, t, 8, 1, E, ctypes.byref(res), st))
        _lib.check(lib.gnnmp_has_self_loops(s, t, 8, E, ctypes.byref(res), st))
        _lib.check(lib.gnnmp_is_sorted(_lib.ptr(self.colptr), 8, N + 1, ctypes.byref(res), st))
        _lib.check(lib.gnnmp_negative_sample(s, t, 8, 1, E, N, E, 0, 3, 77, _lib.ptr(self.neg[0]), _lib.ptr(self.neg[1]), 2 * E,
                                             ctypes.byref(tot), st))
        _lib.check(lib.gnnmp_rand_edge_split(s, t, 8, 1, E, 0, E // 2, 99, *(_lib.ptr(x) for x in self.split), st))
        jobs = ctypes.c_void_p()
        _lib.check(lib.gnnmp_chain_jobs_create(ctypes.byref(jobs), _lib.ptr(self.seg_ptr), GRAPHS, st))
        _lib.check(lib.gnnmp_chain_jobs_destroy(jobs))
        _lib.check(lib.gnnmp_chain_jobs_pack(ctypes.byref(jobs), _lib.ptr(self.seg_ptr), GRAPHS, GRAPHS * PER_GRAPH, PER_GRAPH, 0, st))
        _lib.check(lib.gnnmp_chain_jobs_destroy(jobs))
        members = (ctypes.c_void_p * 2)(self.plan, self.plan)
        cat = ctypes.c_void_p()
        _lib.check(lib.gnnmp_plan_concat(ctypes.byref(cat), members, 2, None, None, 8, 1, st))
        _lib.check(lib.gnnmp_plan_destroy(cat))
        torch.cuda.synchronize()

    def close(self):
        _lib.check(self.lib.gnnmp_plan_destroy(self.plan))


def main():
    su = Setup()
    for name in ("plan_create", "plan_from_csc", "knn_graph", "radius_graph", "sample_neighbors", "induced_subgraph", "unique_append"):
        rc, out = getattr(su, name)()
        assert rc == 0 and out is not None, (name, rc, su.lib.gnnmp_last_error())
    su.others()
    for name in ("plan_create", "plan_from_csc", "knn_graph", "sample_neighbors", "induced_subgraph", "unique_append"):
        rc, _ = getattr(su, name)(bad=True)
        assert rc < 0, name
    su.close()
    torch.cuda.synchronize()
    print("setup_calls ok")


if __name__ == "__main__":
    main()
