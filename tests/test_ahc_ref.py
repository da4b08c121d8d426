"""tests/ahc_ref.py, the NumPy restatement of xv_ahc_cluster, against scipy's average linkage and against the rules the header states:
ties, both stop rules, label numbering, n = 1; and the stability figure the decision-stable GPU cases rest on.  No GPU."""
import numpy as np
import pytest

from tests import ahc_ref as R


def _as_sets(roots):
    groups = {}
    for i, r in enumerate(roots):
        groups.setdefault(r, []).append(i)
    return sorted(tuple(g) for g in groups.values())


def _scipy_partitions(s):
    """The partition after each merge of scipy.cluster.hierarchy.linkage(-S, "average"): average linkage on distances -S is average
    linkage on scores S with the largest average first."""
    from scipy.cluster.hierarchy import linkage
    n = s.shape[0]
    z = linkage(-np.asarray(s, np.float64)[np.triu_indices(n, 1)], "average")
    members = {i: [i] for i in range(n)}
    out = []
    for step, (a, b, _, _) in enumerate(z):
        members[n + step] = members.pop(int(a)) + members.pop(int(b))
        out.append(sorted(tuple(sorted(m)) for m in members.values()))
    return out


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n,k,seed", [(2, 1, 0), (3, 2, 1), (17, 2, 2), (40, 3, 3), (65, 3, 4)])
def test_partitions_equal_scipy_average_linkage_at_every_level(n, k, seed, dtype):
    pytest.importorskip("scipy")
    s, _ = R.clustered_scores(seed, n, k)
    assert R.stability(s, target=1).min() > 8.0      # tie-free, and no decision within fp32 rounding of another
    labels, merges, values = R.cluster(s, target=1, dtype=dtype)
    assert merges.shape == (n - 1, 2) and values.dtype == dtype and (labels == 0).all()
    assert (merges[:, 0] < merges[:, 1]).all()
    got = [_as_sets(p) for p in R.partitions(n, merges)]
    assert got == _scipy_partitions(s)


def test_average_is_the_mean_of_the_member_scores():
    s, _ = R.clustered_scores(7, 12, 2)
    _, merges, values = R.cluster(s, target=1, dtype=np.float64)
    t = R.upper_symmetric(s, np.float64)
    members = {i: [i] for i in range(12)}
    for (a, b), v in zip(merges, values):
        want = t[np.ix_(members[a], members[b])].mean()
        assert abs(v - want) <= 1e-12 * max(1.0, abs(want))
        members[a] = members[a] + members.pop(b)


def test_ties_go_to_the_lowest_a_then_the_lowest_b():
    # a constant matrix: every average stays 0.5 exactly (sums of k halves over k), so every step is a tie over all pairs
    labels, merges, values = R.cluster(np.full((6, 6), 0.5, np.float32), target=1)
    assert merges.tolist() == [[0, 1], [0, 2], [0, 3], [0, 4], [0, 5]] and (values == np.float32(0.5)).all() and (labels == 0).all()
    # block-constant: two blocks {0, 2, 4} and {1, 3, 5} of inner score 0.75, outer 0.25 - ties inside the blocks only
    blk = np.where(np.add.outer(np.arange(6), np.arange(6)) % 2 == 0, 0.75, 0.25).astype(np.float32)
    labels, merges, values = R.cluster(blk, target=1)
    assert merges.tolist() == [[0, 2], [0, 4], [1, 3], [1, 5], [0, 1]]
    assert values.tolist() == [0.75, 0.75, 0.75, 0.75, 0.25]
    # only the upper triangle is read
    low = blk.copy()
    low[np.tril_indices(6, -1)] = -7.0
    assert R.cluster(low, target=1)[1].tolist() == merges.tolist()


def test_stop_rules_and_label_numbering():
    blk = np.where(np.add.outer(np.arange(6), np.arange(6)) % 2 == 0, 0.75, 0.25).astype(np.float32)
    # threshold between the two populations: the blocks, numbered by their smallest members 0 and 1
    labels, merges, _ = R.cluster(blk, threshold=0.5)
    assert labels.tolist() == [0, 1, 0, 1, 0, 1] and len(merges) == 4
    # a threshold equal to a merge value still merges (A >= threshold)
    assert len(R.cluster(blk, threshold=0.75)[1]) == 4 and len(R.cluster(blk, threshold=np.nextafter(np.float32(0.75), np.float32(1)))[1]) == 0
    assert len(R.cluster(blk, threshold=0.25)[1]) == 5
    # a target ignores the threshold
    labels, merges, _ = R.cluster(blk, threshold=9.0, target=2)
    assert labels.tolist() == [0, 1, 0, 1, 0, 1] and len(merges) == 4
    labels, merges, _ = R.cluster(blk, target=6)
    assert labels.tolist() == [0, 1, 2, 3, 4, 5] and merges.shape == (0, 2)
    labels, merges, _ = R.cluster(blk, threshold=-9.0, target=3)
    assert len(merges) == 3 and labels.tolist() == [0, 1, 0, 1, 0, 2]      # {0, 2, 4}, {1, 3}, {5}: ids 0, 1, 5 -> labels 0, 1, 2
    # labels follow ascending cluster id, not merge order
    s = np.zeros((4, 4), np.float32)
    s[2, 3], s[0, 1] = 0.9, 0.8
    labels, merges, _ = R.cluster(s, threshold=0.5)
    assert merges.tolist() == [[2, 3], [0, 1]] and labels.tolist() == [0, 0, 1, 1]


def test_one_row():
    labels, merges, values = R.cluster(np.zeros((1, 1), np.float32))
    assert labels.tolist() == [0] and merges.shape == (0, 2) and values.shape == (0,)
    assert R.stability(np.zeros((1, 1))).shape == (0,)


def test_stability_figures_of_the_gpu_cases():
    """The condition under which tests/test_gpu_ahc.py compares the GPU with the float64 run: every decision at least 8 error bounds
    from every other.  The floors below are what this generator gave when the condition was set (2.91e5, 149.7 and 49.5 at the least);
    larger n is not asked to agree: (130, 4) gives 4.1 on one seed."""
    floor = {(3, 2): 2.9e5, (17, 2): 149.0, (65, 3): 49.0}
    for (n, k), want in floor.items():
        for seed in range(6):
            s, _ = R.clustered_scores(seed, n, k)
            assert R.stability(s, target=1).min() >= want, (n, k, seed)
            assert R.cluster(s, target=1)[1].tolist() == R.cluster(s, target=1, dtype=np.float64)[1].tolist()
    assert min(R.stability(R.clustered_scores(seed, 130, 4)[0], target=1).min() for seed in range(6)) < 8.0
    # a near-tie is seen: two pairs one ulp apart
    s = np.zeros((3, 3), np.float32)
    s[0, 1], s[0, 2] = 0.5, np.nextafter(np.float32(0.5), np.float32(0))
    assert R.stability(s, target=1)[0] < 1.0
