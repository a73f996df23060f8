"""tests/topk_ref.py pinned on the reference's own known answers (GraphNeuralNetworks/test/layers/pool.jl:49-71) and on the rules
include/gnnmp.h states for gnnmp_topk_select_f32 — all on the host."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import topk_ref as R  # noqa: E402


def test_topk_index_known_answers():
    X = np.array([8, 7, 6, 5, 4, 3, 2, 1])
    assert R.topk_index_julia(X, 4).tolist() == [1, 2, 3, 4]
    assert R.topk_index_julia(X.reshape(1, 8), 4).tolist() == [1, 2, 3, 4]          # topk_index(X', 4)
    assert R.topk_index(X, 4).tolist() == [1, 2, 3, 4]
    assert R.topk_index(X.reshape(1, 8), 4).tolist() == [1, 2, 3, 4]


def test_layer_output_shape_of_the_reference_test():
    rng = np.random.default_rng(0)
    N, k, C = 10, 4, 7
    X = rng.random((C, N))
    for A in (rng.random((N, N)) < 0.5, rng.random((N, N))):
        X_, At = R.topk_pool_julia(A, X, rng.standard_normal(C), k)
        assert X_.shape == (C, k) and At.shape == (k, k) and At.dtype == A.dtype


def test_the_sorting_and_the_literal_statement_agree_without_ties():
    rng = np.random.default_rng(1)
    for n in (1, 2, 9, 64, 300):
        y = rng.permutation(n).astype(np.float32)
        for k in (1, 2, n):
            if k <= n:
                assert np.array_equal(R.topk_index(y, k), R.topk_index_julia(y, k))


def test_all_and_first_on_a_tie_across_rank_k():
    y = np.array([3, 5, 5, 5, 1], np.float32)
    keep_f, rank = R.select(y, None, 2, 0.0, R.FIRST)
    keep_a, _ = R.select(y, None, 2, 0.0, R.ALL)
    assert rank.tolist() == [3, 0, 1, 2, 4]                       # equal keys by ascending node id
    assert keep_f.tolist() == [0, 1, 1, 0, 0, 0]                  # exactly k, and keep[N] = 0
    assert keep_a.tolist() == [0, 1, 1, 1, 0, 0]                  # every value at least the k-th largest: the reference's topk_index
    assert R.topk_index_julia(y, 2).tolist() == [2, 3, 4] == R.topk_index(y, 2).tolist()


def test_nan_and_signed_zero_rules():
    nan, inf = np.float32("nan"), np.float32("inf")
    neg_nan = np.array([0xffc00000], np.uint32).view(np.float32)[0]
    y = np.array([nan, -inf, -0.0, 0.0, neg_nan, 1e-45, -1e-45, inf], np.float32)
    key = R.keys(y)
    assert key[0] == 0 and key[4] == 0                            # any NaN: below every number
    assert key[2] == key[3] == 0x80000000                         # -0.0 is +0.0
    assert key[1] > 0 and key[6] < key[2] < key[5] < key[7]       # -Inf above the NaNs; denormals keep their side of zero
    _, rank = R.select(y)
    assert rank.tolist() == [6, 5, 2, 3, 7, 1, 4, 0]              # +Inf, 1e-45, the two zeros by id, -1e-45, -Inf, the NaNs by id
    # the keys are monotone in the value
    rng = np.random.default_rng(2)
    v = np.sort(rng.standard_normal(1000).astype(np.float32))
    assert np.all(np.diff(R.keys(v).astype(np.int64)) >= 0)


def test_k_of_a_member_graph():
    prod = float(np.float32(0.1)) * 30.0                          # (double) ratio * (double) n_g with the record's float ratio
    assert prod != round(prod) and 3.0 < prod < 3.000001 and R.k_of(30, 0, 0.1) == 4
    assert R.k_of(20, 0, 0.1) == 3 and R.k_of(10, 0, 0.1) == 2      # (float) 0.1 lies above 0.1
    assert R.k_of(20, 0, 0.25) == 5 and R.k_of(10, 0, 0.3) == 4     # 0.25 is exact; (float) 0.3 lies above 0.3
    assert R.k_of(7, 0, 0.5) == 4 and R.k_of(1, 0, 0.5) == 1 and R.k_of(1030, 0, 1.0) == 1030
    assert R.k_of(3, 64, 0.0) == 3 and R.k_of(100, 64, 0.0) == 64 and R.k_of(0, 4, 0.0) == 0
    for n in (1, 2, 63, 64, 65, 255, 256, 257, 1030):
        for ratio in (0.1, 0.5, 1.0):
            assert R.k_of(n, 0, ratio) == min(n, math.ceil(float(np.float32(ratio)) * float(n))) >= 1


def test_selection_is_per_member_graph_and_an_empty_one_keeps_nothing():
    ptr = np.array([0, 0, 3, 3, 8])
    y = np.array([1, 3, 2, 9, 9, 9, 1, 0], np.float32)
    keep, rank = R.select(y, ptr, 2, 0.0, R.FIRST)
    assert keep.tolist() == [0, 1, 1, 1, 1, 0, 0, 0, 0]
    assert rank.tolist() == [2, 0, 1, 0, 1, 2, 3, 4]
    keep, _ = R.select(y, ptr, 0, 0.5, R.ALL)                     # k_g = 2 and 3
    assert keep.tolist() == [0, 1, 1, 1, 1, 1, 0, 0, 0]


def test_the_batch_and_its_score_vectors():
    ptr = R.batch_ptr()
    assert np.diff(ptr).tolist() == list(R.SIZES) and ptr[-1] == 1993
    sv = R.score_vectors(ptr)
    assert set(sv) == {"random", "equal", "tie_block", "negative", "specials", "descending", "ascending"}
    sp = sv["specials"]
    assert np.isnan(sp).any() and np.isinf(sp).any() and (sp.view(np.uint32) == 0x80000000).any() and (np.abs(sp[np.isfinite(sp)]) == np.float32(1e-45)).any()
    # the tie block puts equal keys on both sides of rank 4 in every member graph of at least 6 nodes
    for a, b in zip(ptr[:-1], ptr[1:]):
        if b - a >= 6:
            f, _ = R.select(sv["tie_block"][a:b], None, 4, 0.0, R.FIRST)
            al, _ = R.select(sv["tie_block"][a:b], None, 4, 0.0, R.ALL)
            assert f.sum() == 4 and al.sum() > 4


def test_pool_restated_on_exact_inputs():
    """the end-to-end inputs of tests/test_topk_pool.py: small integers and p = (1, 1, 1, 1, 0, 0, 0) — norm 2, every score exact"""
    rng = np.random.default_rng(3)
    x = rng.integers(-3, 4, (12, 7)).astype(np.float64)
    p = np.array([1, 1, 1, 1, 0, 0, 0], np.float64)
    y = R.score64(x, p)
    assert np.array_equal(y, x[:, :4].sum(1) / 2) and np.array_equal(y.astype(np.float32).astype(np.float64), y)
    s0, t0 = rng.integers(0, 12, 30), rng.integers(0, 12, 30)
    idx0, x2, s2, t2, eid = R.topk_pool(x, p, s0, t0, np.array([0, 5, 12]), k=3)
    assert len(idx0) == 6 and x2.shape == (6, 7) and np.all(np.diff(idx0) > 0)
    assert np.array_equal(idx0[s2], s0[eid]) and np.array_equal(idx0[t2], t0[eid])
