"""tests/augment_ref.py — the numpy restatement of remove_nodes / add_edges / add_nodes / perturb_edges that tests/test_plan_edit.py
measures the device against — pinned on the reference's own known answers (GNNGraphs/test/transform.jl:139-282), its mask on the CPU
oracle's dropout_keep, and its pair draw on a chi-square over the ordered pairs."""
import numpy as np
import pytest

import augment_ref as R


def test_remove_nodes_known_answers():
    w = np.array([0.1, 0.2, 0.3, 0.4], np.float32)
    s2, t2, w2, n2, nid, eid = R.remove_nodes([1, 1, 2, 3], [2, 3, 4, 5], w, 5, [1])          # transform.jl:197-225
    assert (s2.tolist(), t2.tolist(), n2) == ([1, 2], [3, 4], 4)
    assert w2.tolist() == w[[2, 3]].tolist() and nid.tolist() == [1, 2, 3, 4] and eid.tolist() == [2, 3]
    s2, t2, w2, n2, nid, eid = R.remove_nodes([1, 5, 2, 3], [2, 3, 4, 5], w, 5, [1, 4])       # transform.jl:228-254
    assert (s2.tolist(), t2.tolist(), n2) == ([3, 2], [2, 3], 3)
    assert w2.tolist() == w[[1, 3]].tolist() and nid.tolist() == [1, 2, 4] and eid.tolist() == [1, 3]
    # repeats and any order: sort(union(...))
    again = R.remove_nodes([1, 5, 2, 3], [2, 3, 4, 5], w, 5, [4, 1, 4, 1])
    assert again[0].tolist() == [3, 2] and again[3] == 3
    # 0-based indices, the same graph
    z = R.remove_nodes([0, 4, 1, 2], [1, 2, 3, 4], w, 5, [0, 3], base=0)
    assert (z[0].tolist(), z[1].tolist(), z[3]) == ([2, 1], [1, 2], 3)


def test_remove_nodes_p_ends():
    s, t = [1, 1, 2, 3], [2, 3, 4, 5]                                                        # transform.jl:257-273
    for seed in (0, 42, 0xDEADBEEF12345):
        none = R.remove_nodes_p(s, t, None, 5, 1.0, seed)
        assert none[3] == 0 and len(none[0]) == 0 and len(none[4]) == 0
        full = R.remove_nodes_p(s, t, None, 5, 0.0, seed)
        assert full[3] == 5 and full[0].tolist() == s and full[1].tolist() == t and full[5].tolist() == [0, 1, 2, 3]


def test_mask_is_the_oracles_dropout_keep():
    from oracle import oracle as orc
    for seed, p, n in ((0xDEADBEEF12345, 0.3, 300), (7, 0.5, 33), (1 << 63, 0.1, 1), (12345, 0.0, 64), (99, 0.999, 257)):
        want = np.asarray(orc.dropout_keep(seed, p, n, 1)).reshape(n) != 0
        assert np.array_equal(R.keep_mask(seed, p, n), want), (seed, p, n)


def test_add_edges_known_answers():
    s, t = [1, 1, 2, 3], [2, 3, 4, 5]
    s2, t2, w2, n2 = R.add_edges(s, t, None, 5, [1], [4])                                    # transform.jl:141-152
    assert len(s2) == 5 and n2 == 5 and w2 is None
    assert sorted(s2[t2 == 4].tolist()) == [1, 2]                                            # inneighbors(gnew, 4)
    s2, t2, w2, n2 = R.add_edges([], [], None, 0, [1, 3], [2, 1])                            # adding new nodes, :160-167
    assert (n2, len(s2)) == (3, 2) and s2[t2 == 1].tolist() == [3] and t2[s2 == 1].tolist() == [2]
    w = [1.0, 2.0, 3.0, 4.0]                                                                 # also add weights, :168-183
    assert R.add_edges(s, t, None, 5, [1], [4], [5.0])[2].tolist() == [1.0, 1.0, 1.0, 1.0, 5.0]
    assert R.add_edges(s, t, w, 5, [1], [4], [5.0])[2].tolist() == w + [5.0]
    assert R.add_edges(s, t, w, 5, [1], [4], None)[2].tolist() == w + [1.0]
    same = R.add_edges(s, t, w, 5, [], [])                                                   # length(snew) == 0: g itself
    assert same[0].tolist() == s and same[2] is w and same[3] == 5
    with pytest.raises(AssertionError):
        R.add_edges(s, t, None, 5, [0], [4])                                                 # @assert minimum(snew) >= 1


def test_perturb_edges_count_and_add_nodes():
    s, t = [1, 2, 3, 4, 5], [2, 3, 4, 5, 1]                                                  # transform.jl:187-193
    s2, t2, w2, n2 = R.perturb_edges(s, t, None, 5, 0.5, 42)
    assert len(s2) == 8 and n2 == 5 and s2[:5].tolist() == s and t2[:5].tolist() == t
    assert np.all(s2[5:] != t2[5:]) and s2[5:].min() >= 1 and s2[5:].max() <= 5 and t2[5:].min() >= 1 and t2[5:].max() <= 5
    assert R.perturb_edges(s, t, None, 5, 0.0, 42)[0].tolist() == s
    assert R.perturb_edges(s, t, [1.0] * 5, 5, 0.5, 42)[2].tolist() == [1.0] * 8             # new edges weigh 1
    with pytest.raises(AssertionError, match="perturb_ratio must be between 0 and 1"):
        R.perturb_edges(s, t, None, 5, 1.5, 42)
    with pytest.raises(AssertionError, match="at least 2 nodes"):
        R.perturb_edges([1], [1], None, 1, 1.0, 42)
    assert R.add_nodes(6, 5) == 11                                                           # transform.jl:275-282


# the 0.999 quantile of chi-square at 55 degrees of freedom (Wilson-Hilferty: 55 (1 - 2 / 495 + 3.0902 sqrt(2 / 495))^3 = 93.17)
CHI2_55_999 = 93.17


@pytest.mark.parametrize("seed", [1, (42 << 32) | 7, 0xDEADBEEF12345])
def test_pair_draw_is_uniform_over_the_ordered_pairs(seed):
    N, m = 8, 56 * 200
    s, t = R.rand_pairs(seed, m, N)
    assert not np.any(s == t) and s.min() >= 0 and s.max() < N and t.min() >= 0 and t.max() < N
    counts = np.bincount(s * N + t, minlength=N * N).reshape(N, N)
    assert np.all(np.diag(counts) == 0)
    obs = counts[~np.eye(N, dtype=bool)]
    chi2 = float(((obs - 200.0) ** 2 / 200.0).sum())
    print(f"seed {seed}: chi2 = {chi2:.2f}")
    assert chi2 < CHI2_55_999
