"""gnnmp_dense_f32's routing on the GPU against tests/golden/dense_routes_v1.json: what gnnmp_debug_dense_route reported, shape by shape,
row count by row count, misalignment by misalignment and knob setting by knob setting, in the library BEFORE the routing moved into the
planner of csrc/dense_route.h (the file names the commit).  Every recorded row is called again with real buffers at the recorded
offsets: the hook's eight ints must equal the recorded ones, and a second call into a second buffer must give the same bits.  The grid
is that of tests/dense_route_cases.py; tests/test_dense_route_cpu.py holds the planner itself to the same rows without a GPU."""
import contextlib
import ctypes

import pytest

import dense_route_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rows_by_knob():
    g, rows = C.load_golden()
    by = {name: [] for name, _ in C.KNOBS}
    names = {id(kv): name for name, kv in C.KNOBS}
    for shape, N, off, kv, info in rows:
        if N <= 4096:                                         # (the rows above are the CPU test's: dense_wreg's threshold)
            by[names[id(kv)]].append((shape, N, off, info))
    return g, by


@pytest.fixture(scope="module")
def operands():
    """per shape: seeded x1, x2, W1, W2, bias and two output buffers, each 64 floats longer than the largest row count called here needs"""
    import torch
    assert torch.cuda.is_available()
    import gnnmp
    gnnmp.load()
    cache = {}

    def get(shape):
        if shape not in cache:
            K1, K2, Dout = shape
            g = torch.Generator(device="cuda")
            g.manual_seed(1000 * K1 + 10 * K2 + Dout)
            nmax = max(n for n in C.gpu_ns(shape) if n <= 4096)
            rnd = lambda n: torch.randn(n, device="cuda", generator=g)
            cache[shape] = (rnd(nmax * K1 + 64), rnd(nmax * K2 + 64) if K2 else None, rnd(Dout * K1) * 0.1, rnd(Dout * K2) * 0.1 if K2 else None,
                            rnd(Dout), torch.empty(nmax * Dout + 64, device="cuda"), torch.empty(nmax * Dout + 64, device="cuda"))
            assert all(t is None or t.data_ptr() % 256 == 0 for t in cache[shape])
        return cache[shape]
    return get


@pytest.mark.parametrize("setting", [name for name, _ in C.KNOBS])
def test_recorded_routes_and_run_to_run_bits(rows_by_knob, operands, setting):
    import torch
    from gnnmp import _lib as L
    g, by = rows_by_knob
    rows = by[setting]
    assert torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count == g["cus"], "recorded on another CU count"
    lib = L.load()
    info_c = (ctypes.c_int * 8)()
    stream = L.stream_ptr()
    mismatches = torch.zeros(len(rows), dtype=torch.int64, device="cuda")
    wrong = []
    at = lambda t, off: ctypes.c_void_p(t.data_ptr() + 4 * off) if t is not None else None
    with contextlib.ExitStack() as stack:
        for k, v in dict(C.KNOBS)[setting].items():
            stack.enter_context(L.tuned(k, v))                # the value the library held comes back on the way out
        for i, ((K1, K2, Dout), N, (o1, o2, oo), info) in enumerate(rows):
            x1, x2, W1, W2, b, ya, yb = operands((K1, K2, Dout))
            for y in (ya, yb):
                L.check(lib.gnnmp_dense_f32(at(x1, o1), L.ptr(W1), K1, K1, at(x2, o2), L.ptr(W2), K2, K2, 0, L.ptr(b), 1, at(y, oo), N, Dout, stream))
                L.check(lib.gnnmp_debug_dense_route(info_c))
                if list(info_c) != info:
                    wrong.append(((K1, K2, Dout), N, (o1, o2, oo), list(info_c), info))
            if N:
                va, vb = ya[oo:oo + N * Dout].view(torch.int32), yb[oo:oo + N * Dout].view(torch.int32)
                mismatches[i] = torch.count_nonzero(va != vb)
    assert not wrong, f"{len(wrong)} rows took another route than recorded (shape, N, offsets, hook, recorded): {wrong[:5]}"
    bad = mismatches.nonzero().flatten().tolist()
    assert not bad, f"{len(bad)} rows differ between two calls, first {rows[bad[0]][:3]}"
