"""The numpy restatements of ppr_diffusion (tests/ppr_ref.py), without a GPU: known answers of the reference's formula, the pivoting and
the singular case of the elimination csrc/ppr.hip runs, the condition on every input of tests/test_ppr.py (cond(M) < 10 in float64), and
the figure K of the device's bar: for every such input the error of the float32 restatement of the kernel's elimination, in units of the
reference's own float32 error, is at most K / 2."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ppr_ref as R  # noqa: E402

f32 = np.float32
FORMS = (R.ref64, R.lapack32, R.restate32)


def close(got, want):
    return np.allclose(np.asarray(got, np.float64), np.asarray(want, np.float64), rtol=1e-6, atol=1e-7)


# ---- known answers -----------------------------------------------------------------------------------------------------------------
def test_one_node_without_edges_gives_an_empty_result():
    for form in FORMS:
        assert form(*R._g([], [], 1), 0.85).shape == (0,)


@pytest.mark.parametrize("w", [0.25, 1.0, 3.0])
def test_one_node_with_a_self_loop(w):
    a = f32(0.85)
    want = float(a) / (1.0 + (float(a) - 1.0) * w)
    for form in FORMS:
        got = form(*R._g([0], [0], 1, [w]), 0.85)
        assert got.shape == (1,) and close(got, [want]), form.__name__


def test_a_two_cycle_by_hand():
    """M = [1 -0.5; -0.5 1], 0.5 * inv(M) = [2/3 1/3; 1/3 2/3]: both edges are off the diagonal"""
    g, alpha = R.TWO_CYCLE
    for form in FORMS:
        assert close(form(*g, alpha), [1 / 3, 1 / 3]), form.__name__


def test_alpha_one_gives_one_on_self_loops_and_zero_elsewhere():
    g, alpha = R.known_cases()["alpha1"]
    want = (g[0] == g[1]).astype(np.float64)
    assert want.sum() == 3 and len(want) == 6
    for form in FORMS:
        assert np.array_equal(np.asarray(form(*g, alpha), np.float64), want), form.__name__


def test_every_copy_of_a_multi_edge_receives_the_same_value_and_the_copies_are_summed():
    doubled = R._g([0, 0, 1, 2], [1, 1, 2, 0], 3, [0.5, 0.25, 1.0, 1.0])
    merged = R._g([0, 1, 2], [1, 2, 0], 3, [0.75, 1.0, 1.0])
    assert R.matrix32(*doubled, 0.85)[1, 0] == f32(f32(0.85) - f32(1.0)) * f32(0.75)                  # A[t, s] = 0.5 + 0.25
    for form in FORMS:
        d, m = form(*doubled, 0.85), form(*merged, 0.85)
        assert d[0] == d[1], form.__name__
        assert np.array_equal(d[1:], m), form.__name__
    once = R.ref64(*R._g([0, 1, 2], [1, 2, 0], 3, [0.5, 1.0, 1.0]), 0.85)
    assert abs(once[0] - R.ref64(*doubled, 0.85)[0]) > 1e-3                      # the copy counts


def test_the_matrix_is_indexed_target_source_and_no_column_is_normalised():
    g = R._g([0, 0], [1, 2], 3, [1.0, 1.0])                                       # 0 -> 1, 0 -> 2
    M = R.matrix32(*g, 0.85)
    am1 = f32(f32(0.85) - f32(1.0))
    assert M[1, 0] == am1 and M[2, 0] == am1 and M[0, 1] == 0 and M[0, 2] == 0     # column 0 sums to 1 + 2 (alpha - 1): not normalised
    assert np.array_equal(np.diag(M), np.ones(3, f32))


def test_a_batch_equals_its_members_taken_alone():
    for weights in (False, True):
        ms = R.members(weights)
        g, off, eoff = R.batch(weights)
        assert len(off) == len(ms) + 3 and np.sum(np.diff(off) == 0) == 2 and off[-1] == g[2] == sum(R.SIZES)
        whole64, whole32 = R.ref64(*g, R.ALPHA), R.restate32(*g, R.ALPHA)
        for i, m in enumerate(ms):
            assert np.allclose(whole64[eoff[i]:eoff[i + 1]], R.ref64(*m, R.ALPHA), rtol=1e-12, atol=1e-14), i
            # the elimination of the whole block-diagonal matrix does to a member's elements exactly what its own elimination does
            assert np.array_equal(whole32[eoff[i]:eoff[i + 1]], R.restate32(*m, R.ALPHA)), i


# ---- pivoting, singular --------------------------------------------------------------------------------------------------------------
def test_the_pivoting_case_swaps_and_succeeds():
    g, alpha = R.PIVOT
    M = R.matrix32(*g, alpha)
    assert M[0, 0] == 0 and np.array_equal(M, np.array([[0, -0.5], [-0.5, 1]], f32))
    assert np.array_equal(R.inverse32(M), np.array([[-4, -2], [-2, 0]], f32))
    for form in FORMS:
        assert np.array_equal(np.asarray(form(*g, alpha), f32), R.PIVOT_ANSWER), form.__name__


def test_the_lowest_row_wins_a_tie():
    """column 0 holds 1, -1, 1: the pivot is row 0 — no exchange; were it row 1 or 2 the elimination order, hence the bits, would differ"""
    M = np.array([[1, 2, 0], [-1, 1, 3], [1, 0, 5]], f32)
    got = R.inverse32(M)
    assert np.allclose(got.astype(np.float64), np.linalg.inv(M.astype(np.float64)), rtol=1e-6, atol=1e-7)


def test_the_exchange_input_exchanges_rows_at_almost_every_step():
    """the random inputs are nearly diagonally dominant (M = I - 0.15 A) and never exchange; this one does, across the two waves of a
    pivot column: what the device's pivot reduction, its substitution of the old a_kk and its multi-exchange column map are run on"""
    g, alpha = R.known_cases()["exchange70"]
    ex = []
    inv = R.inverse32(R.matrix32(*g, alpha), ex)
    assert g[2] == 70 and len(ex) >= 60 and all(p > k for k, p in ex)
    assert sum(k < 64 <= p for k, p in ex) >= 5                                    # the pivot found beyond the first 64 rows
    M = R.matrix32(*g, alpha).astype(np.float64)
    assert np.abs(inv.astype(np.float64) @ M - np.eye(70)).max() < 1e-5
    for name in R.random_cases():                                                  # and the claim about the others
        gg, al = R.random_cases()[name]
        none = []
        R.inverse32(R.matrix32(*gg, al), none)
        assert none == [], name


def test_the_singular_case_reports_the_zero_pivot():
    g, alpha = R.SINGULAR
    assert np.array_equal(R.matrix32(*g, alpha), np.zeros((1, 1), f32))
    with pytest.raises(R.Singular) as e:
        R.restate32(*g, alpha)
    assert e.value.step == 0
    # after pivoting: a zero on the diagonal alone is not singular (the pivoting case), a zero COLUMN below the diagonal is
    with pytest.raises(R.Singular) as e:
        R.inverse32(np.array([[1, 2], [2, 4]], f32))
    assert e.value.step == 1


def test_the_restated_inverse_is_an_inverse():
    rng = np.random.default_rng(5)
    for n in (1, 2, 3, 17, 40):
        M = (np.eye(n) + 0.3 * rng.standard_normal((n, n))).astype(f32)           # needs exchanges
        inv = R.inverse32(M)
        assert inv.dtype == f32
        assert np.abs(inv.astype(np.float64) @ M.astype(np.float64) - np.eye(n)).max() < 1e-4 * np.linalg.cond(M.astype(np.float64)), n


# ---- the condition on the inputs, and K --------------------------------------------------------------------------------------------------
def test_every_gpu_input_is_well_conditioned():
    refs = R.references()
    assert {f"n{n}_{tag}" for n in R.SIZES for tag in "uw"} | {"batch_u", "batch_w", "n150_w", "large300_w", "pivot", "two_cycle", "alpha1", "exchange70"} == set(refs)
    for name, (g, alpha, r64, lap) in refs.items():
        c = R.cond(*g, alpha)
        assert c < R.COND_BAR, (name, c)
        assert r64.shape == lap.shape == (len(g[0]),) and lap.dtype == f32, name
        if name in R.random_cases():
            assert alpha == R.ALPHA and (g[3] is None or (g[3].min() >= 0.1 and g[3].max() <= 1.0)), name
            assert len(g[0]) <= 4 * g[2], name                                       # mean in-degree <= 4
    g = R.large_graph()
    assert g[2] == 300 and len(g[0]) == 1200
    assert R.opt_in_graph()[2] == 150
    for m in R.members(True)[2:]:                                                    # from 5 nodes on: a multi-edge, a self loop, an isolated node
        s, t, n, _ = m
        assert (s[0], t[0]) == (s[1], t[1]) and s[2] == t[2] and n - 1 not in s and n - 1 not in t


def test_k_is_twice_the_worst_ratio_of_the_restatement():
    """THE FIGURE: the float32 restatement of the kernel's elimination is within K / 2 of the float64 reference on every device input, in
    units of max(max|lapack32 - ref64|, 2^-24 max|ref64|); the device is held to K.  K is never taken from a device."""
    worst = 0.0
    for name, (g, alpha, r64, lap) in R.references().items():
        ra = R.ratio(R.restate32(*g, alpha), lap, r64)
        print(f"{name}: nodes {g[2]}, edges {len(g[0])}, ratio {ra:.3f}")
        assert ra <= R.K / 2, (name, ra)
        worst = max(worst, ra)
    assert isinstance(R.K, int) and R.K == math.ceil(2 * worst), (R.K, worst)        # the rule, pinned: neither short nor padded
