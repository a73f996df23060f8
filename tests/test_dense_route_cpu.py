"""csrc/dense_route.h — the planner of the dense family (which kernel, which template instance, what launch geometry a gnnmp_dense_f32
call gets) — on the CPU: the same header under plain g++ (no HIP), driven by tests/c_harness/dense_route_check.cpp over the grid of
tests/dense_route_cases.py.  Every line is compared with that module's `restated`, written by hand from the five host paths the planner
replaced, and checked against the invariants the kernels rely on; the 16 entries of tests/test_dense_fallbacks.py: TABLE come out as
written there; every row of tests/golden/dense_routes_v1.json (what the library BEFORE the planner reported on an MI355X through
gnnmp_debug_dense_route) comes out of the planner too.  A second build of the driver runs under -fsanitize=address,undefined."""
import ast
import os
import subprocess

import pytest

import dense_route_cases as C

ROOT = C.ROOT
LDS = 160 * 1024


def _build(tmp_path_factory, name, extra):
    exe = str(tmp_path_factory.mktemp(name) / "dense_route_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", *extra, "-I" + os.path.join(ROOT, "graphneuralnetworks.jl_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c_harness", "dense_route_check.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _build(tmp_path_factory, "plain", [])


def _line(shape, N, facts, cus, kn):
    K1, K2, Dout = shape
    return "%d %d %d %d %d %d %d %d %d %d %d %d %d %d" % (N, K1, K2, Dout, *facts, cus, kn.get(C.GENERIC, 0), kn.get(C.DENSE_SPLIT, 0),
                                                        kn.get(C.VARIANT, 0), kn.get(C.T16_WAVES, 0), kn.get(C.PREFETCH, 17))


def _plan(exe, queries):
    """queries: (shape, N, facts, cus, knobs) -> one route dict each"""
    r = subprocess.run([exe], input="\n".join(_line(*q) for q in queries) + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(queries)
    return [dict(zip(C.FIELDS, map(int, ln.split()))) for ln in lines]


ALL16 = [(a, b, c, d) for a in (1, 0) for b in (1, 0) for c in (1, 0) for d in (1, 0)]
# under a non-default knob setting: everything aligned, nothing aligned, and each fact off alone (out 16-byte off takes 128 with it)
SOME = [(1, 1, 1, 1), (0, 0, 0, 0), (0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 0), (1, 1, 1, 0)]


def _grid():
    """every shape x N x knob setting x CU count; all 16 alignment combinations at default knobs on 256 CUs, SOME under the other knob
    settings, the two extremes at the other CU counts (no predicate looks at CUs and alignment together)"""
    for shape in C.SHAPES:
        for N in C.NS:
            for name, kn in C.KNOBS:
                for cus in C.CUS:
                    for facts in ((ALL16 if name == "default" else SOME) if cus == 256 else SOME[:2]):
                        yield (shape, N, facts, cus, kn)


def _check_invariants(q, r):
    (K1, K2, Dout), N, facts, cus, kn = q
    k = r["kernel"]
    assert r["lds_bytes"] <= LDS, (q, r)
    if N == 0:
        assert k == C.NONE
        return
    assert k != C.NONE
    if k == C.SPLIT:
        dp = r["ncb"] * 32
        assert r["ncb"] in (2, 4) and 1 <= r["waves"] <= 8 and r["grid_y"] * dp >= Dout > (r["grid_y"] - 1) * dp, (q, r)
        assert 1 <= r["grid_x"] <= cus and r["grid_x"] * r["waves"] <= -(-N // 32) + r["waves"] - 1, (q, r)
        assert (r["k0c"] == 0 or (r["k0c"], r["k1c"]) == (K1, K2)) and bool(r["k1c"]) == bool(K2), (q, r)
    elif k == C.T16:
        dp = r["ncb"] * 16
        assert r["ncb"] in (2, 4, 6, 7, 8) and 1 <= r["waves"] <= (12 if r["ncb"] == 8 else 16), (q, r)
        assert r["grid_y"] * dp >= Dout > (r["grid_y"] - 1) * dp and 1 <= r["grid_x"] <= cus, (q, r)
        assert r["kq1"] == -1 or (4 * r["kq1"], 4 * r["kq2"]) == (K1, K2), (q, r)
    elif k == C.WREG:
        assert Dout == 256 and r["waves"] == 8 and (r["k0c"], r["k1c"]) == (K1, K2) and 1 <= r["grid_x"] <= cus and r["grid_y"] == 1, (q, r)
    elif k == C.NARROW:
        assert Dout <= r["nout"] <= 8 and r["grid_x"] * 32 >= N, (q, r)
    elif k == C.WLDS:
        nt = r["nt_full"] if r["full"] else r["rem_nt"]
        wbytes = r["ktot_pad"] * (nt * 32 + 1) * 4
        assert r["waves"] in (4, 8) and r["tw"] in (64, 128) and 0 <= r["rem_nt"] <= 4 and r["nt_full"] in (0, 2, 4), (q, r)
        assert wbytes + r["waves"] * r["region"] * 4 + 16 == r["lds_bytes"], (q, r)       # the 4 pipe tokens after the regions
        # an epilogue pass writes min(tp * 32, widest tile) columns into rows of `old` floats inside the region's rows.  (tp stays 4 when
        # the whole tile fits, so "tp * 32 <= region columns" holds only where tp was cut down: Dout = 2 has tp = 4 in a 104-column region.)
        widest = r["tw"] if r["full"] else Dout % r["tw"]
        assert r["region"] % 32 == 0 and 1 <= r["tp"] <= 4 and min(r["tp"] * 32, widest) <= r["old"] <= r["region"] // 32, (q, r)
        assert r["tp"] == 4 or r["tp"] * 32 <= r["region"] // 32, (q, r)
        assert r["old"] % 4 == 0 and r["old"] <= r["region"] // 32 and r["xld"] % 2 == 1 and r["xld"] <= r["region"] // 32, (q, r)
        assert r["ks"] % 4 == 0 and 0 < r["ks"] <= 128, (q, r)
        assert r["full"] * r["tw"] + (r["rem_nt"] * 32 if r["rem_nt"] else 0) >= Dout == r["full"] * r["tw"] + Dout % r["tw"], (q, r)
        assert r["ktot_pad"] == (K1 + 1) // 2 * 2 + (K2 + 1) // 2 * 2 and 1 <= r["grid_x"] <= cus, (q, r)
        if r["prefetch"]:
            assert K2 == 0 and K1 % 4 == 0 and facts[0] and r["ks"] >= K1, (q, r)          # what the kernel's register prefetch assumes
    else:
        assert k == C.MFMA and r["grid_x"] * 128 >= N and r["grid_y"] * 128 >= Dout, (q, r)


def test_planner_matches_the_restated_host_paths_and_its_invariants(exe):
    queries = list(_grid())
    got = _plan(exe, queries)
    seen = set()
    for q, r in zip(queries, got):
        want = C.restated(*q)
        assert r == want, (q, {f: (r[f], want[f]) for f in C.FIELDS if r[f] != want[f]})
        _check_invariants(q, r)
        seen.add((r["kernel"], r["ncb"], r["k0c"], r["k1c"], r["maxb"], r["kq1"], r["nout"], r["nt_full"], r["rem_nt"], r["kq2"]))
    # every compile-time instance the host paths name is reached by the grid (VAR apart: four per split instance)
    assert {s[1:4] for s in seen if s[0] == C.SPLIT} == {(4, 16, 16), (4, 100, 100), (4, 0, 1), (4, 100, 0), (4, 128, 0), (4, 0, 0),
                                                         (2, 128, 128), (2, 0, 1), (2, 0, 0)}
    assert {(s[1], s[4], s[5], s[9]) for s in seen if s[0] == C.T16} == {
        (8, 7, 25, 0), (8, 8, 32, 0), (8, 7, 25, 25), (8, 8, 32, 32), (8, 1, 4, 4), (8, 8, -1, -1), (7, 7, 25, 0), (7, 8, -1, -1), (6, 8, -1, -1),
        (4, 8, -1, -1), (2, 8, -1, -1)}
    assert {s[2:4] for s in seen if s[0] == C.WREG} == set(C.WREG_PAIRS)
    assert {s[6] for s in seen if s[0] == C.NARROW} == {2, 4, 8}
    assert {s[7] for s in seen if s[0] == C.WLDS} == {0, 2, 4} and {s[8] for s in seen if s[0] == C.WLDS} == {0, 1, 2, 3, 4}
    assert {s[0] for s in seen} == set(range(7))


def test_fallback_table_comes_out_as_written(exe):
    """tests/test_dense_fallbacks.py: TABLE, read from that file (the module itself is marked gpu), at its threshold N = 256"""
    src = open(os.path.join(ROOT, "tests", "test_dense_fallbacks.py")).read()
    node = next(n for n in ast.parse(src).body if isinstance(n, ast.Assign) and getattr(n.targets[0], "id", "") == "TABLE")
    table = eval(compile(ast.Expression(node.value), "TABLE", "eval"), {"dict": dict})
    assert table == C.FALLBACK_TABLE and len(table) == 16
    shapes = list(table)
    for cus in C.CUS:
        got = _plan(exe, [(s, 256, (1, 1, 1, 1), cus, {}) for s in shapes])
        for (K1, K2, Dout), r in zip(shapes, got):
            chunks = -(-max((K1 + 1) & ~1, (K2 + 1) & ~1) // r["ks"])
            assert r["kernel"] == C.WLDS
            assert dict(tw=r["tw"], waves=r["waves"], chunks=chunks, tp=r["tp"], nt=r["rem_nt"], pf=r["prefetch"]) == table[(K1, K2, Dout)]
    got = _plan(exe, [(s, 293, (1, 1, 1, 1), 256, {}) for s in C.MFMA_ONLY])
    assert [r["kernel"] for r in got] == [C.MFMA, C.MFMA]


def test_planner_reproduces_the_recorded_routes(exe):
    """every row the library before the planner reported on the GPU: the hook's eight ints (zero after `kernel` unless dense_wlds_kernel)"""
    g, rows = C.load_golden()
    assert len(g["commit"]) == 40 and len(rows) > 50000
    got = _plan(exe, [(shape, N, C.facts_of(off), g["cus"], kn) for shape, N, off, kn, _ in rows])
    for (shape, N, off, kn, info), r in zip(rows, got):
        hook = [r[f] for f in C.FIELDS[:8]] if r["kernel"] == C.WLDS else [r["kernel"]] + [0] * 7
        assert hook == info, (shape, N, off, kn, hook, info)


def test_driver_is_clean_under_the_sanitizers(tmp_path_factory):
    exe = _build(tmp_path_factory, "asan", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    queries = [(shape, N, facts, cus, kn) for shape in C.SHAPES for N in (0, 31, 256, 32768) for facts in ((1, 1, 1, 1), (0, 0, 0, 0))
               for cus in C.CUS for _, kn in C.KNOBS[:6]]
    got = _plan(exe, queries)
    assert len(got) == len(queries)
