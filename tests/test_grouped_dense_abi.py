"""The grouped dense exports (csrc/dense_grouped.hip) at the C ABI.  Without a device: header, SYMBOLS, library and records agree, the planning
header compiles with g++, every refusal comes before any launch.  On the device: the memory contract and the capture-replay check over the
cases of tests/grouped_dense_cases.py with the registry's own helpers (as tests/test_topk_abi.py runs them)."""
import ctypes
import os
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_cases as A  # noqa: E402
import grouped_dense_cases as GC  # noqa: E402  (registers the cases in A.TABLE)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = (GC.FWD, GC.GRAD)
WSP, ROUTE = "gnnmp_grouped_dense_grad_workspace", "gnnmp_debug_grouped_dense_route"


def test_header_symbols_library_and_records():
    import gnnmp
    from gnnmp import _lib
    h = A.parse_header()
    header = open(os.path.join(ROOT, "include", "gnnmp.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    assert all(name in h[0] and name in _lib.SYMBOLS and name in exported for name in ALL + (WSP, ROUTE))
    assert header.index(f"int {GC.GRAD}(") < header.index("GNNMP_INTERNAL") < header.index(f"int {ROUTE}(")
    why = {}
    need = A.must_be_covered(h[0], _lib.SYMBOLS, h.records, why)
    for name in ALL:          # launch-only (their comment never speaks of a wait or an allocation), owed to the table and in it
        assert [p[0] for p in h[0][name]] == ["job", "N", "G", "K", "Dout", "stream"] and h[0][name][0][2]
        assert not any(A.WAITS_OR_ALLOCATES.search(t) for t in A.header_comments_of(name)), name
        assert name in need and why[name] == "record" and name in A.capturable()
    for rtype, st, size in (("gnnmp_grouped_dense_t", _lib.GroupedDenseJob, 96), ("gnnmp_grouped_dense_grad_t", _lib.GroupedDenseGradJob, 88)):
        assert A.struct_of(rtype) is st and [f[0] for f in h.records[rtype]] == [n for n, _ in st._fields_] and ctypes.sizeof(st) == size
    assert callable(gnnmp.grouped_dense) and callable(gnnmp.grouped_dense_ad)
    # the planning header has no HIP in it: g++ alone, warnings as errors (the routes it plans are asserted in tests/test_grouped_route_cpu.py)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "graphneuralnetworks.jl_amd", "csrc"),
                    "-include", "dense_grouped_route.h", "-x", "c++", os.devnull], check=True)


P_ = lambda v: ctypes.c_void_p(0x1000 * v) if v else None      # never dereferenced: the call must refuse first  # noqa: E731


def test_refusals_come_before_any_launch():
    import torch
    import gnnmp
    from gnnmp import _lib
    lib = _lib.load()
    EINVAL, OK, err = _lib.EINVAL, _lib.OK, lib.gnnmp_last_error

    def fwd(job=True, x=1, ldx=8, W=2, ws=32, ldw=8, lay=0, bias=None, bs=0, sp=3, act=0, out=4, ldo=4, N=10, G=2, K=8, Dout=4):
        j = _lib.GroupedDenseJob(P_(x), ldx, P_(W), ws, ldw, lay, P_(bias), bs, P_(sp), act, P_(out), ldo)
        return lib.gnnmp_grouped_dense_f32(ctypes.byref(j) if job else None, N, G, K, Dout, None)

    def grad(job=True, dz=1, lddz=4, x=2, ldx=8, sp=3, dW=4, dws=32, db=5, dbs=4, w=6, wf=10 ** 6, N=10, G=2, K=8, Dout=4):
        j = _lib.GroupedDenseGradJob(P_(dz), lddz, P_(x), ldx, P_(sp), P_(dW), dws, P_(db), dbs, P_(w), wf)
        return lib.gnnmp_grouped_dense_grad_w_f32(ctypes.byref(j) if job else None, N, G, K, Dout, None)
    size = b"bad size"
    bad_fwd = ((dict(job=False), b"null job"), (dict(N=-1), size), (dict(G=-1), size), (dict(K=0), size), (dict(Dout=0), size),
               (dict(K=2 ** 20 + 1, ldx=2 ** 21, ldw=2 ** 21), size), (dict(lay=2), b"w_layout"), (dict(act=2), b"act"), (dict(ldx=7), b"ldx"),
               (dict(ldo=3), b"ldo"), (dict(ldw=7), b"ldw"), (dict(lay=1, ldw=3), b"ldw"), (dict(ws=-1), b"w_stride"), (dict(bias=5, bs=3), b"bias_stride"),
               (dict(G=0), b"no group"), (dict(x=None), b"null pointer"), (dict(sp=None), b"null pointer"), (dict(out=None), b"null pointer"))
    bad_grad = ((dict(job=False), b"null job"), (dict(N=-1), size), (dict(G=-1), size), (dict(K=0), size), (dict(Dout=2 ** 16 + 1, lddz=2 ** 17), size),
                (dict(G=2 ** 22), size), (dict(dW=None, db=None), b"nothing to compute"), (dict(lddz=3), b"lddz"), (dict(ldx=7), b"ldx"),
                (dict(dws=31), b"dw_stride"), (dict(dbs=3), b"db_stride"), (dict(G=0), b"no group"), (dict(sp=None), b"null pointer"),
                (dict(w=None), b"null pointer"), (dict(x=None), b"null pointer"), (dict(wf=2 * (32 + 4) - 1), b"workspace too small"))
    for call, table in ((fwd, bad_fwd), (grad, bad_grad)):
        for bad, word in table:
            assert call(**bad) == EINVAL and word in err(), bad
    assert fwd(N=0) == OK and fwd(N=0, G=0) == OK and grad(N=0, G=0) == OK      # nothing to do: nothing is launched (there is no device here)
    assert lib.gnnmp_grouped_dense_grad_workspace(10, 2, 4, 8) == 2 * (32 + 4) and lib.gnnmp_grouped_dense_grad_workspace(10, 0, 4, 8) == 0
    info = (ctypes.c_int * 4)(7, 7, 7, 7)
    assert lib.gnnmp_debug_grouped_dense_route(info) == OK and list(info) == [0, 0, 0, 0]      # the last call returned before a launch
    with pytest.raises(TypeError, match="Float64 is not supported"):                           # by name, before the device is asked for
        gnnmp.grouped_dense(torch.zeros(4, 4, dtype=torch.float64), torch.zeros(1, 4, 4), [0, 4])


@pytest.mark.gpu
@pytest.mark.parametrize("export", ALL)
def test_the_memory_contract(export):
    import torch
    from gnnmp import _lib
    lib = _lib.load()
    plans, failures, runs = A.Plans(lib), [], 0
    for case in A.TABLE[export](A.Ctx(int(A.parse_header()[1]["GNNMP_MIN_LONG_ROW"]))):
        sets = [("natural alignment", None, None)] + ([("side stream", None, torch.cuda.Stream())] if "side" in case.tags else [])
        for tag, nbytes in A.SHIFTS.items() if "align" in case.tags else ():
            names = [a.name for a in case.arrs if nbytes % a.dtype.itemsize == 0]
            sets += [(f"{n}+{tag}", {n: nbytes}, None) for n in names] + [(f"all+{tag}", {n: nbytes for n in names}, None)]
        for what, shifts, stream in sets:
            rc, slab, host = A.run_case(lib, case, plans, shifts=shifts, stream=stream)
            runs += 1
            failures += [f"{case.export}[{case.sid}] {what}: {p}" for p in A.verify(case, rc, slab, host)]
    assert not failures and runs >= 30, "\n".join(failures)


@pytest.mark.gpu
@pytest.mark.parametrize("export", ALL)
def test_capture_replay_new_values_and_back_to_back(export):
    import torch
    import test_abi_graph_capture as C
    from gnnmp import _lib
    C._require_working_capture()
    thr = int(A.parse_header()[1]["GNNMP_MIN_LONG_ROW"])                  # (the cases take no plan: the threshold steers nothing here)
    (c0,), (c1,) = C._capture_cases(A.Ctx(thr, variant=0), export), C._capture_cases(A.Ctx(thr, variant=1), export)
    problems, differ, floats = C._same_call(c0, c1)
    assert not problems and differ and floats, (export, problems)
    problems = C._record_and_replay(_lib.load(), c0, c1, A.Plans(_lib.load()), torch.cuda.Stream())
    assert not problems, f"{export}[{c0.sid}]:\n  " + "\n  ".join(problems)
