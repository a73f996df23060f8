"""The tuning knobs have one source of truth: the table of csrc/knobs.h, the values inside the library (gnnmp_tune / gnnmp_tune_get).
gnnmp/knobs.py mirrors the names by hand and is pinned to the header here; nothing on the host keeps a copy of a value.  CPU only:
the library loads and its knobs work without a GPU (tests/test_abi.py)."""
import ctypes
import os
import re
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "graphneuralnetworks.jl_amd", "csrc", "knobs.h")
DEFAULTS = {1: -1, 3: 1, 7: 17}          # the parent commit's: every other knob starts at 0


def header_table():
    """[(name, index, default)] of the X(NAME, index, default, "meaning") lines"""
    rows = re.findall(r"^\s*X\((\w+), (-?\d+), (-?\d+), \"", open(HEADER).read(), flags=re.M)
    return [(name, int(index), int(default)) for name, index, default in rows]


def header_variants():
    return {name: int(value) for name, value in re.findall(r"^\s*VARIANT_(\w+) = (\d+),", open(HEADER).read(), flags=re.M)}


@pytest.fixture(scope="module")
def L():
    from gnnmp import _lib
    _lib.load()
    return _lib


def test_python_names_equal_the_header_table():
    from gnnmp.knobs import Knob, Variant
    import gnnmp
    table = header_table()
    assert [index for _, index, _ in table] == list(range(len(table)))          # dense, in order: entry i is knob i
    assert {name: index for name, index, _ in table} == {k.name: int(k) for k in Knob}
    assert len(table) == 24 and table[8][0] == "GAT_FAST_EXP" and table[23][0] == "CHUNK_SLOTS"      # slot 8 stays, reserved
    assert {index: default for _, index, default in table if default != 0} == DEFAULTS
    assert header_variants() == {name: int(v) for name, v in Variant.__members__.items()}
    assert {"CHAIN_8_WAVES": 1, "SPLIT_SERIAL_TILES": 16, "SPLIT_DIRECT_STORES": 32, "NO_WREG": 64, "TWO_KERNEL_FOLD": 128,
            "WREG_SMALL": 512}.items() <= header_variants().items()
    assert gnnmp.Knob is Knob and gnnmp.Variant is Variant
    from gnnmp import _lib
    assert (_lib.KNOB_TGCN, _lib.KNOB_EDGE_DOT_GRAD, _lib.KNOB_HETERO) == (20, 21, 22)


def test_defaults_of_a_fresh_library(L, tmp_path):
    """a private copy of the library under another name: whatever earlier tests of this process set does not reach it"""
    copy = str(tmp_path / "libgnnmp_fresh.so")
    shutil.copy(L.LIB_PATH, copy)
    lib = ctypes.CDLL(copy)
    n = len(header_table())
    for k in range(n):
        v, d = ctypes.c_int(-99), ctypes.c_int(-99)
        assert lib.gnnmp_tune_get(k, ctypes.byref(v), ctypes.byref(d)) == L.OK
        assert v.value == d.value == DEFAULTS.get(k, 0), k
    assert [d for _, _, d in header_table()] == [DEFAULTS.get(k, 0) for k in range(n)]


def test_set_get_round_trip(L):
    import gnnmp
    lib = L.load()
    n = len(header_table())
    v = ctypes.c_int(-99)
    for bad in (-1, n):
        assert lib.gnnmp_tune(bad, 1) == L.EINVAL and b"bad knob" in lib.gnnmp_last_error()
        assert lib.gnnmp_tune_get(bad, ctypes.byref(v), None) == L.EINVAL and b"bad knob" in lib.gnnmp_last_error()
        assert v.value == -99
        with pytest.raises(gnnmp.GnnmpError):
            gnnmp.knob(bad)
    assert lib.gnnmp_tune_get(7, None, None) == L.OK
    d = ctypes.c_int(-99)
    assert lib.gnnmp_tune_get(7, None, ctypes.byref(d)) == L.OK and d.value == 17
    # a value set behind the host's back is the value the host reads: nothing in Python mirrors the library's state
    k = gnnmp.Knob.FUSED_WAVES
    before = gnnmp.knob(k)
    try:
        assert lib.gnnmp_tune(int(k), 5) == L.OK
        assert gnnmp.knob(k) == 5 and gnnmp.knob(int(k)) == 5
        gnnmp.tune(int(k), -3)                              # plain integers keep working
        assert lib.gnnmp_tune_get(int(k), ctypes.byref(v), ctypes.byref(d)) == L.OK and (v.value, d.value) == (-3, 0)
    finally:
        lib.gnnmp_tune(int(k), before)


def test_tuned_restores_what_the_library_held(L):
    import gnnmp
    K, V = gnnmp.Knob, gnnmp.Variant
    lib = L.load()
    assert lib.gnnmp_tune(int(K.DENSE_PREFETCH), 33) == L.OK           # set behind the host's back: tuned() restores THIS, not a default
    try:
        with gnnmp.tuned(K.DENSE_PREFETCH, 1):
            assert gnnmp.knob(K.DENSE_PREFETCH) == 1
        assert gnnmp.knob(K.DENSE_PREFETCH) == 33
        with pytest.raises(ZeroDivisionError):
            with gnnmp.tuned(K.DENSE_PREFETCH, 2):
                assert gnnmp.knob(K.DENSE_PREFETCH) == 2
                1 // 0
        assert gnnmp.knob(K.DENSE_PREFETCH) == 33
        with gnnmp.tuned(K.CHAIN, -1):
            with gnnmp.tuned(K.CHAIN, 1):
                with gnnmp.tuned(K.DENSE_PREFETCH, 4):
                    assert (gnnmp.knob(K.CHAIN), gnnmp.knob(K.DENSE_PREFETCH)) == (1, 4)
                assert (gnnmp.knob(K.CHAIN), gnnmp.knob(K.DENSE_PREFETCH)) == (1, 33)
            assert gnnmp.knob(K.CHAIN) == -1
        assert gnnmp.knob(K.CHAIN) == 0
        with gnnmp.tuned_bits(K.VARIANT, set=V.WREG_SMALL | V.TWO_KERNEL_FOLD):
            assert gnnmp.knob(K.VARIANT) == 512 + 128
            with gnnmp.tuned_bits(K.VARIANT, set=V.NO_WREG, clear=V.TWO_KERNEL_FOLD):
                assert gnnmp.knob(K.VARIANT) == 512 + 64
            assert gnnmp.knob(K.VARIANT) == 512 + 128
        assert gnnmp.knob(K.VARIANT) == 0
    finally:
        lib.gnnmp_tune(int(K.DENSE_PREFETCH), 17)


def test_release_build_refuses_the_ablation_knob(L):
    """knob 13's values skip phases of kernels on purpose: only a library built with -DGNNMP_EXPERIMENTS takes them"""
    import gnnmp
    lib = L.load()
    k = int(gnnmp.Knob.T16_DEBUG)
    assert k == 13 and lib.gnnmp_tune(k, 1) == L.EUNSUPPORTED
    assert b"GNNMP_EXPERIMENTS" in lib.gnnmp_last_error()
    assert gnnmp.knob(gnnmp.Knob.T16_DEBUG) == 0
    with pytest.raises(gnnmp.GnnmpError, match="GNNMP_EXPERIMENTS"):
        gnnmp.tune(gnnmp.Knob.T16_DEBUG, 2)
    assert lib.gnnmp_tune(k, 0) == L.OK and gnnmp.knob(k) == 0


def test_an_abi_case_puts_its_knobs_back(L):
    """abi_cases.call restores the value a knob had, not 0: knob 1 starts at -1"""
    import abi_cases as A
    lib = L.load()
    v = ctypes.c_int()
    assert lib.gnnmp_tune_get(1, ctypes.byref(v), None) == L.OK and v.value == -1
    case = A.Case("gnnmp_tune_get", "knob-restore", [1, ctypes.byref(v), None], None, knobs={1: 0})
    assert A.call(lib, case, case.args) == L.OK and v.value == 0                 # the call itself ran under the case's setting
    assert lib.gnnmp_tune_get(1, ctypes.byref(v), None) == L.OK and v.value == -1
