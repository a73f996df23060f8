"""csrc/scratch.h — DevBuf (the scoped owner of device scratch on the set-up path), the prep cache behind it, alloc_into and grow — on the
CPU: the same header under plain g++ (no HIP), with the counting stand-ins of tests/c_harness/scratch_check.cpp for hipMalloc / hipFree.
Checked there: one give-back per alloc on normal exit, early return and after a move; release() suppresses it; a failed alloc leaves the
buffer empty; a prep-cache buffer is freed unless synced() was called, parked with it, and the next fitting request on the same device gets
the same block; grow keeps the buffer when it is large enough, frees before it allocates otherwise, and leaves (nullptr, 0) after a failure."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_devbuf_prep_cache_and_grow_with_counting_stand_ins(tmp_path):
    exe = str(tmp_path / "scratch_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "graphneuralnetworks.jl_amd", "csrc"),
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c_harness", "scratch_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-3000:]
    for what in ("give-back on exit, early return, move", "release / alloc_into", "failed alloc", "prep cache parks only after synced()", "grow"):
        assert "ok  " + what in r.stdout, r.stdout[-3000:]
    assert "all " in r.stdout and "checks passed" in r.stdout
