"""csrc/dense_grouped_route.h — the planner of the grouped dense exports (which kernel, which instance, what launch geometry) — on the CPU:
the same header under plain g++ (no HIP), driven by tests/c_harness/grouped_route_check.cpp, as tests/test_dense_route_cpu.py drives
dense_route.h.  Every route of a sweep over N, G, K, Dout, the alignment facts and the CU count is checked against the invariants the
kernels of csrc/dense_grouped.hip rely on (each read from the kernel source and stated beside its assertion); the cases of
tests/test_grouped_dense_geometry.py come out, at 256 CUs, as tests/grouped_dense_cases.py writes them down — a device with another CU
count then fails there with a route to compare, not with a mystery.  A second build of the driver runs under -fsanitize=address,undefined."""
import itertools
import os
import subprocess

import pytest

import grouped_dense_cases as GC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS = 160 * 1024
NONE, T16, FMA, GRADW16, GRADW_FMA = 0, 1, 2, 3, 4
FIELDS = ("kernel", "ncb", "waves", "tiles_per_block", "grid_x", "grid_y", "lds_bytes", "g_kernel", "slabs", "g_waves", "tiles_per_wave",
          "g_grid_x", "g_grid_y", "g_grid_z", "fold_y", "workspace")
NS = (0, 1, 15, 16, 17, 171, 739, 4096, 5130, 41040, 200000, 2 ** 24)
GS = (1, 2, 12, 360, 2880, 4096)
KS = (2, 4, 5, 20, 24, 68, 100, 192, 272, 320, 640, 1264, 1284)
DOUTS = (3, 4, 7, 12, 40, 52, 72, 100, 112, 128, 132, 300, 5000)
CUS = (1, 64, 256, 304)


def _build(tmp_path_factory, name, extra):
    exe = str(tmp_path_factory.mktemp(name) / "grouped_route_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", *extra, "-I" + os.path.join(ROOT, "graphneuralnetworks.jl_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c_harness", "grouped_route_check.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _build(tmp_path_factory, "plain", [])


def _plan(exe, queries):
    """queries: (N, G, K, Dout, x_al16, out_al16, want_dw, cus) -> one dict of FIELDS each"""
    r = subprocess.run([exe], input="".join("%d %d %d %d %d %d %d %d\n" % q for q in queries), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(queries)
    return [dict(zip(FIELDS, map(int, ln.split()))) for ln in lines]


def _grid():
    """the whole product of the sizes at 256 CUs with everything aligned and dW wanted; the other alignment facts, db alone and the other CU
    counts on every third shape (no predicate of the planner looks at two of them together but `T16 needs both facts`, which all four
    combinations of the thinned part cover)"""
    for i, (N, G, K, Dout) in enumerate(itertools.product(NS, GS, KS, DOUTS)):
        yield (N, G, K, Dout, 1, 1, 1, 256)
        if i % 3 == 0:
            for xa, oa, dw, cus in ((0, 1, 1, 256), (1, 0, 0, 256), (0, 0, 1, 64), (1, 1, 1, 1), (1, 1, 0, 64), (1, 1, 1, 304), (0, 0, 0, 304)):
                yield (N, G, K, Dout, xa, oa, dw, cus)


def t16_lds(K, ncb):
    return (((K // 4) + 3) & ~3) * ncb * 16 * 16 + ncb * 16 * 4                # grouped_t16_lds: the image's rows of ncb * 16 float4, the bias


def _check(q, r):
    N, G, K, Dout, xa, oa, dw, cus = q
    # ---- forward ----
    assert (r["kernel"] == NONE) == (N == 0), (q, r)
    if r["kernel"] == T16:
        assert K % 4 == 0 and Dout % 4 == 0 and xa and oa, (q, r)              # float4 loads of x rows, float4 stores of out rows
        assert r["ncb"] in (2, 4, 6, 7, 8), (q, r)                             # the instances the export's switch launches
        assert r["lds_bytes"] == t16_lds(K, r["ncb"]) <= LDS, (q, r)           # bias4 = img + t16_img_rows(K) * DP lies inside the allocation
        assert 1 <= r["waves"] and 64 * r["waves"] <= (768 if r["ncb"] >= 8 else 1024), (q, r)      # __launch_bounds__(t16_max_threads(NCB))
        dp, sr = r["ncb"] * 16, r["tiles_per_block"] * r["waves"] * 16
        assert r["grid_y"] * dp >= Dout > (r["grid_y"] - 1) * dp, (q, r)       # ncols = min(DP, Dout - n0) is positive in every column tile
        assert r["tiles_per_block"] >= 1 and r["grid_x"] * sr >= N > (r["grid_x"] - 1) * sr, (q, r)  # every row in a block, no block idle
    elif r["kernel"] == FMA:
        assert 1 <= r["tiles_per_block"] <= 256, (q, r)
        assert r["grid_x"] * r["tiles_per_block"] >= N > (r["grid_x"] - 1) * r["tiles_per_block"] and r["grid_y"] == 1, (q, r)
        # the only ways off the MFMA core: a shape or an alignment it cannot take, or no instance whose image fits LDS
        assert K % 4 or Dout % 4 or not xa or not oa or t16_lds(K, 2) > LDS, (q, r)
    if N:
        assert 1 <= r["grid_x"] <= 2 ** 31 - 1 and 1 <= r["grid_y"] <= 65535, (q, r)
    # ---- the weight gradient ----
    S = r["slabs"]
    assert 1 <= S <= 1024 and r["g_grid_x"] == G * S and r["workspace"] == G * S * (Dout * K + Dout), (q, r)
    assert 1 <= r["g_grid_x"] <= 2 ** 31 - 1 and 1 <= r["g_grid_y"] <= 65535 and 1 <= r["g_grid_z"] <= 65535 and 1 <= r["fold_y"] <= 1024, (q, r)
    if r["g_kernel"] == GRADW16:
        assert dw and K % 4 == 0 and Dout % 4 == 0 and xa, (q, r)
        assert 1 <= r["g_waves"] <= 4, (q, r)                                  # __launch_bounds__(256)
        assert r["g_grid_z"] * r["g_waves"] * r["tiles_per_wave"] * 16 >= K, (q, r)      # k0 of the last wave's last tile reaches K
        assert 1 <= r["tiles_per_wave"] <= 4, (q, r)                           # grouped_gradw16_kernel<TO, 4>: acc[TO][4], kcol[4]
        assert r["g_grid_y"] * 128 >= Dout > (r["g_grid_y"] - 1) * 128, (q, r)   # o0 = blockIdx.y * 128; <4, 4> when Dout <= 64, else <8, 4>
    else:
        assert r["g_kernel"] == GRADW_FMA and 1 <= r["g_grid_y"] <= 64 and r["g_grid_z"] == 1, (q, r)
        assert not (dw and K % 4 == 0 and Dout % 4 == 0 and xa), (q, r)


def test_planner_keeps_what_the_kernels_rely_on(exe):
    queries = list(_grid())
    got = _plan(exe, queries)
    for q, r in zip(queries, got):
        _check(q, r)
    # the sweep reaches every forward instance, the step-down, the aligned shape no instance fits, and both gradient kernels with a split in y and z
    assert {r["ncb"] for r in got if r["kernel"] == T16} == {2, 4, 6, 7, 8}
    assert any(r["kernel"] == T16 and r["ncb"] == 7 and q[3] == 128 for q, r in zip(queries, got))
    assert any(r["kernel"] == FMA and q[2] == 1284 and q[3] == 4 and q[4] and q[5] for q, r in zip(queries, got))
    assert {r["tiles_per_wave"] for r in got if r["g_kernel"] == GRADW16} == {1, 2, 3, 4}
    assert any(r["g_kernel"] == GRADW16 and r["g_grid_y"] > 1 and r["g_grid_z"] > 1 for r in got)
    assert any(r["g_kernel"] == GRADW_FMA and r["g_grid_y"] == 64 for r in got) and max(r["slabs"] for r in got) > 4


def test_tiles_per_wave_stays_within_the_instance_up_to_the_largest_k(exe):
    """every K the export admits (a multiple of 4 up to 2^16): a wave never owns more than the four 16-column tiles <TO, 4> has registers for"""
    queries = [(4096, 12, K, 12, 1, 1, 1, 256) for K in range(4, 2 ** 16 + 1, 4)]
    for q, r in zip(queries, _plan(exe, queries)):
        assert r["g_kernel"] == GRADW16 and 1 <= r["tiles_per_wave"] <= 4 and 1 <= r["g_grid_z"] <= 65535, (q, r)
        assert r["g_grid_z"] * r["g_waves"] * r["tiles_per_wave"] * 16 >= q[2], (q, r)


def _sizes(s):
    return s() if callable(s) else s


def test_geometry_cases_come_out_as_written_at_256_cus(exe):
    """tests/grouped_dense_cases.py: GEOM_FWD and GEOM_GRAD, the routes tests/test_grouped_dense_geometry.py reaches on an MI355X"""
    fwd = [(sum(_sizes(c[1])), len(_sizes(c[1])), c[2], c[3], int(c[7] % 4 == 0 and c[8] == 0), int(c[7] % 4 == 0), 1, 256) for c in GC.GEOM_FWD]
    for c, q, r in zip(GC.GEOM_FWD, fwd, _plan(exe, fwd)):
        assert (r["kernel"], r["ncb"], r["waves"], r["tiles_per_block"], r["grid_x"], r["grid_y"]) == c[10], (c[0], q, r)
        N, why = q[0], c[9]
        if why in ("multiwave", "persistent_multiwave"):
            assert r["waves"] >= 2 and (why != "multiwave" or GC.check_cut(c[1], r["waves"])), (c[0], r)
        if why in ("persistent", "persistent_multiwave"):
            assert r["grid_x"] * r["waves"] * 16 < N and r["tiles_per_block"] >= 2, (c[0], r)
        if why == "fma_multiblock":
            assert r["grid_x"] > 1, (c[0], r)
    grad = [(sum(c[1]), len(c[1]), c[2], c[3], int(c[6] % 4 == 0 and c[7] == 0), 1, int(c[4]), 256) for c in GC.GEOM_GRAD]
    for c, q, r in zip(GC.GEOM_GRAD, grad, _plan(exe, grad)):
        got = (r["g_kernel"], r["slabs"], r["g_waves"], r["tiles_per_wave"], r["g_grid_x"], r["g_grid_y"], r["g_grid_z"], r["fold_y"])
        assert got == c[9] and r["slabs"] >= c[8], (c[0], q, r)
    by_id = {c[0]: c[9] for c in GC.GEOM_GRAD}
    assert by_id["kz2_oy2"][2:4] == (4, 3) and by_id["kz2_oy2"][5:7] == (2, 2)      # 17 k-tiles over 2 x 4 waves of 3: two waves of z = 1 idle
    # the Δx of tests/test_grouped_dense.py's cut_multiwave case: the forward with K and Dout swapped keeps four waves a block
    (r,) = _plan(exe, [(sum(GC.CUT), len(GC.CUT), 12, 24, 1, 1, 1, 256)])
    assert (r["kernel"], r["ncb"], r["waves"]) == (T16, 2, 4)


def test_driver_is_clean_under_the_sanitizers(tmp_path_factory):
    exe = _build(tmp_path_factory, "asan", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    queries = list(_grid())
    assert len(_plan(exe, queries)) == len(queries)
