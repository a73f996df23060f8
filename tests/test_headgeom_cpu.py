"""csrc/headgeom.h — which lanes hold one attention head (the rule the one-pass attention forward and its two pullbacks share) — on the
CPU: the same header under plain g++ (no HIP), driven by tests/c_harness/headgeom_check.cpp over H in 1..8 + {12, 16, 32, 64}, C in 1..80 +
{96, 100, 128, 256} and vec0 in {1, 2, 4}.  Every line is compared with the restatement below, written by hand from the three copies the
header replaced (attn_conv_impl, gat_conv_grad_impl, attn_conv_grad_impl), and checked against the invariants the kernels rely on."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HS = list(range(1, 9)) + [12, 16, 32, 64]
CS = list(range(1, 81)) + [96, 100, 128, 256]
VECS = [1, 2, 4]


def _is_pow2(n):
    return n >= 1 and n & (n - 1) == 0


def _restated(H, C, vec0):
    """(vec, lanes, log2g, lph, lph_code, fits_wave, arm16, arm64) as the three host paths computed them, each in its own words"""
    vec = vec0
    while vec > 1 and C % vec != 0:
        vec //= 2
    lanes = H * C // vec
    log2g = 0
    while (1 << log2g) < lanes:
        log2g += 1
    lph = C // vec
    if H == 1 and lanes <= 64:
        # attn_conv_impl / attn_conv_grad_impl: 1 << log2g; gat_conv_grad_impl: its own doubling loop — the same number
        spill = 1
        while spill < lanes:
            spill *= 2
        assert spill == 1 << log2g
        lph = spill
    code = lph if _is_pow2(lph) else (0x10000 | (log2g << 8) | lph)
    # the forward's ladder compared the CODE with 1, 2, ..., 64 for vec 4; the pullbacks switched on the raw count 1, 2, ..., 16 for vec 4
    arm64 = code if vec == 4 and code in (1, 2, 4, 8, 16, 32, 64) else 0
    arm16 = lph if vec == 4 and lph in (1, 2, 4, 8, 16) else 0
    return vec, lanes, log2g, lph, code, int(lanes <= 64), arm16, arm64


def test_head_geometry_matches_the_restated_rule_and_its_invariants(tmp_path):
    exe = str(tmp_path / "headgeom_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "graphneuralnetworks.jl_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c_harness", "headgeom_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-3000:]
    got = {}
    for ln in r.stdout.splitlines():
        key, val = ln.split(" : ")
        got[tuple(int(t) for t in key.split())] = tuple(int(t) for t in val.split())
    assert len(got) == len(HS) * len(CS) * len(VECS)
    for H in HS:
        for C in CS:
            for vec0 in VECS:
                g = got[(H, C, vec0)]
                assert g == _restated(H, C, vec0), (H, C, vec0, g)
                vec, lanes, log2g, lph, code, fits, arm16, arm64 = g
                assert vec in (1, 2, 4) and vec <= vec0 and C % vec == 0
                assert lanes * vec == H * C
                assert fits == int(lanes <= 64)
                if fits:
                    assert (1 << log2g) >= lanes and (log2g == 0 or lanes > (1 << (log2g - 1)))
                    if H == 1:
                        assert lph == 1 << log2g
                assert bool(code & 0x10000) == (not _is_pow2(lph))
                if code & 0x10000:
                    assert code & 0xff == lph and (code >> 8) & 0xff == log2g   # what group_sum<0> decodes
                else:
                    assert code == lph
