"""The data-dependent error exits of the host set-up path — the ones a kernel's own range flag reports (the kernels clamp the index and set
a flag: nothing is read or written out of bounds, these are ordinary status returns) — at tiny shapes (tools/setup_calls.py: N = 100,
E = 1 000, 64 seed nodes, 32 graphs x 16 points with d = 3):

    gnnmp_plan_create        validate = 1, one source index = N + 1                    GNNMP_EBOUNDS
    gnnmp_plan_from_csc      a decreasing colptr                                       GNNMP_EBOUNDS
    gnnmp_sample_neighbors   capacity one short of the total                           GNNMP_EINVAL
    gnnmp_induced_subgraph   capacity one short of the total                           GNNMP_EINVAL
    gnnmp_unique_append      a candidate = N + 1                                       GNNMP_EBOUNDS
    gnnmp_knn_graph_f32      k = 16 on graphs of 16 points, no self loops              GNNMP_EBOUNDS

(gnnmp_negative_sample asked for more negatives than exist is NOT an error exit: gnnmp.h — "possibly fewer than asked for (as in the
reference) when the trials run out" — so it has no case here.)

For each: the status is the one gnnmp.h documents; a correct call straight after the failing one, on the same stream, gives the bytes of
the same correct call made before any failing call; and once one failing call has warmed the scratch cache and the block pool, 50 more
leave the device's free memory exactly where it was — every exit gives back what it took."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

gpu = pytest.mark.gpu

GNNMP_EINVAL, GNNMP_EBOUNDS = -1, -2          # include/gnnmp.h
CASES = [("plan_create", GNNMP_EBOUNDS), ("plan_from_csc", GNNMP_EBOUNDS), ("sample_neighbors", GNNMP_EINVAL),
         ("induced_subgraph", GNNMP_EINVAL), ("unique_append", GNNMP_EBOUNDS), ("knn_graph", GNNMP_EBOUNDS)]


@pytest.fixture(scope="module")
def setup():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import setup_calls
    su = setup_calls.Setup()
    # the correct calls BEFORE any failing call, once, shared by the cases
    su.before = {}
    for name, _ in CASES:
        rc, out = getattr(su, name)()
        assert rc == 0, (name, su.lib.gnnmp_last_error())
        su.before[name] = out
    yield su
    su.close()


@gpu
@pytest.mark.parametrize("name,status", CASES)
def test_error_exit_reports_cleans_up_and_leaks_nothing(setup, name, status):
    import torch
    call = getattr(setup, name)
    rc, _ = call(bad=True)
    assert rc == status, (rc, setup.lib.gnnmp_last_error())
    assert setup.lib.gnnmp_last_error() != b""
    rc, after = call()
    assert rc == 0, setup.lib.gnnmp_last_error()
    before = setup.before[name]
    assert len(after) == len(before)
    for a, b in zip(after, before):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), f"{name}: a correct call after the failing one differs"
    # the failing call above warmed the scratch cache and the pool
    call(bad=True)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(50):
        rc, _ = call(bad=True)
        assert rc == status
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info()[0] == free0, f"{name}: 50 failing calls moved the free device memory by {free0 - torch.cuda.mem_get_info()[0]} bytes"
