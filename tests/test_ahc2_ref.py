"""tests/ahc2_ref.py, the NumPy restatement of the two-pass clustering, against tests/ahc_ref.py (the yardstick of xv_ahc_cluster) and
against the rules the header states: the floor and the threshold, the seeded sizes, the order of the cluster sums, the subset rule, and
the condition under which one pass and two passes give the same partition.  No GPU."""
import numpy as np
import pytest

from tests import ahc_ref as R
from tests import ahc2_ref as R2


def _same(got, want):
    assert got[1].tolist() == want[1].tolist()
    assert got[2].view(np.int32).tolist() == want[2].view(np.int32).tolist()
    assert got[0].tolist() == want[0].tolist()


@pytest.mark.parametrize("n,k,seed", [(2, 1, 0), (3, 2, 1), (17, 2, 2), (40, 3, 3), (65, 3, 4)])
def test_unit_sizes_and_the_old_stop_rules_give_the_old_restatement(n, k, seed):
    """tests/test_ahc_ref.py's own cases: with unit sizes, floor = max(target, 1) and threshold -inf, or floor 1 and the threshold, the
    seeded restatement is tests/ahc_ref.py's run, bit for bit."""
    s, _ = R.clustered_scores(seed, n, k)
    full = R.cluster(s, target=1)
    for target in sorted({1, 2, n // 2 + 1, n}):
        if target <= n:
            _same(R2.cluster_from_scores(s, floor=target), R.cluster(s, target=target))
            _same(R2.cluster_from(R.upper_symmetric(s, np.float32), np.ones(n), floor=target), R.cluster(s, target=target))
    for threshold in [-2.0, 2.0] + [float(v) for v in full[2][::max(1, n // 5)]]:
        _same(R2.cluster_from_scores(s, floor=1, threshold=threshold), R.cluster(s, threshold=threshold))


def test_ties_and_block_constant_scores_as_the_old_restatement():
    blk = np.where(np.add.outer(np.arange(6), np.arange(6)) % 2 == 0, 0.75, 0.25).astype(np.float32)
    for s in (np.full((6, 6), 0.5, np.float32), blk):
        _same(R2.cluster_from_scores(s), R.cluster(s, target=1))
        _same(R2.cluster_from_scores(s, threshold=0.5), R.cluster(s, threshold=0.5))
    low = blk.copy()
    low[np.tril_indices(6, 0)] = np.nan      # only the upper triangle is read
    _same(R2.cluster_from_scores(low), R.cluster(blk, target=1))


def test_floor_and_threshold_stop_together():
    s, _ = R.clustered_scores(3, 40, 3)
    values = R.cluster(s, target=1)[2]
    assert values[30] < values[29]
    mid = 0.5 * (float(values[29]) + float(values[30]))
    assert len(R2.cluster_from_scores(s, floor=20, threshold=mid)[1]) == 20      # the floor first
    assert len(R2.cluster_from_scores(s, floor=5, threshold=mid)[1]) == 30       # the threshold first
    assert len(R2.cluster_from_scores(s, floor=40, threshold=-np.inf)[1]) == 0   # floor = n: nothing
    assert len(R2.cluster_from_scores(s, floor=1, threshold=float(values[30]))[1]) == 31      # A >= threshold still merges
    labels = R2.cluster_from_scores(s, floor=38)[0]
    assert labels.max() == 37 and sorted(set(labels.tolist())) == list(range(38))


def test_seeded_sizes_divide_the_sums_and_large_products_round_once():
    # three clusters: the averages, not the sums, decide
    t = np.array([[0, 30, 40], [30, 0, 10], [40, 10, 0]], np.float32)
    labels, merges, values = R2.cluster_from(t, [10, 1, 20])      # 30 / 10 = 3, 40 / 200 = 0.2, 10 / 20 = 0.5
    assert merges.tolist() == [[0, 1], [0, 2]] and values.tolist() == [3.0, np.float32(50.0) / np.float32(220.0)]
    # a product above 2^24 that fp32 does not hold: 5001 * 4999 = 24999999 -> 25000000 (round to nearest even)
    assert float(np.float32(5001 * 4999)) == 25000000.0
    t = np.array([[0, 1e7], [1e7, 0]], np.float32)
    _, _, values = R2.cluster_from(t, [5001, 4999])
    assert values[0] == np.float32(1e7) / np.float32(25000000.0)


def test_cluster_sums_are_the_sums_of_the_member_scores_in_the_stated_order():
    rs = np.random.RandomState(0)
    s = rs.randn(23, 23).astype(np.float32)
    labels = np.array([0, 1, 0, 2, 1, 0, 3, 3, 2, 0, 1, 4, 4, 0, 2, 1, 3, 0, 4, 2, 1, 0, 3])      # interleaved, numbered by smallest member
    lists = R2.member_lists(labels)
    t, sizes = R2.cluster_sums(s, lists)
    assert sizes.tolist() == np.bincount(labels).tolist() and t.dtype == np.float32
    assert np.array_equal(t, t.T) and (np.diag(t) == 0).all()
    e = R.upper_symmetric(s, np.float64)
    for a in range(5):
        for b in range(a + 1, 5):
            acc = 0.0
            for i in lists[a]:          # the order, spelt out: rows of A ascending, in each the members of B ascending
                row = 0.0
                for j in lists[b]:
                    row = row + e[i, j]
                acc = acc + row
            assert t[a, b] == np.float32(acc)
    low = s.copy()
    low[np.tril_indices(23, 0)] = np.nan
    assert np.array_equal(R2.cluster_sums(low, lists)[0], t)
    # all singletons: the seed is the symmetric matrix itself; one cluster: a single zero
    assert np.array_equal(R2.cluster_sums(s, [np.array([i]) for i in range(23)])[0], R.upper_symmetric(s, np.float32))
    assert R2.cluster_sums(s, [np.arange(23)])[0].tolist() == [[0.0]]


def test_seed_of_singletons_continues_as_one_pass():
    """The seed of all singletons is T itself, so a seeded run from it is the run from the scores."""
    s, _ = R.clustered_scores(2, 17, 2)
    t, sizes = R2.cluster_sums(s, [np.array([i]) for i in range(17)])
    _same(R2.cluster_from(t, sizes), R.cluster(s, target=1))


def test_subset_rule():
    assert R2.subsets(2, 2) == [0, 2] and R2.subsets(2, 2048) == [0, 2]
    assert R2.subsets(2048, 2048) == [0, 2048]
    assert R2.subsets(2049, 2048) == [0, 1025, 2049]                       # first_pass_max_points + 1: two halves, not 2048 + 1
    assert R2.subsets(4096, 2048) == [0, 2048, 4096] and R2.subsets(6144, 2048) == [0, 2048, 4096, 6144]      # exact multiples
    assert R2.subsets(4097, 2048) == [0, 1366, 2732, 4097]
    assert R2.subsets(33, 32) == [0, 17, 33] and R2.subsets(64, 32) == [0, 32, 64] and R2.subsets(5, 2) == [0, 2, 4, 5]
    for n in range(2, 200):
        for cap in (2, 3, 7, 32, 64):
            b = R2.subsets(n, cap)
            sizes = np.diff(b)
            assert b[0] == 0 and b[-1] == n and (sizes >= 1).all() and sizes.max() <= cap and len(sizes) == -(-n // cap)
            assert (sizes[:-1] == sizes[0]).all() and sizes[-1] <= sizes[0]


def blobs(seed, n, k, dim=16, spread=0.04):
    """Well-separated speakers that recur all along the recording: unit-length offsets at mutual cosine below 0.6, a within-speaker spread
    of `spread` per dimension (offsets several times the spread), the speaker of row i drawn at random.  -> (cosine scores float32, who)."""
    rs = np.random.RandomState(seed)
    while True:
        means = rs.randn(k, dim)
        means /= np.linalg.norm(means, axis=1, keepdims=True)
        if k == 1 or (means @ means.T - np.eye(k)).max() < 0.6:
            break
    who = rs.randint(0, k, n)
    who[:k] = np.arange(k)
    x = means[who] + spread * rs.randn(n, dim)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return (x @ x.T).astype(np.float32), who


def _partition(labels):
    seen = {}
    return [seen.setdefault(int(l), len(seen)) for l in labels]


@pytest.mark.parametrize("n,k,cap", [(70, 3, 32), (97, 2, 32), (150, 4, 32), (130, 3, 64)])
def test_two_passes_and_one_pass_agree_on_well_separated_blobs(n, k, cap):
    """A condition on the inputs, not a tolerance: every same-speaker score above every other one, speakers in every subset."""
    s, who = blobs(n, n, k)
    same = np.equal.outer(who, who)
    upper = np.triu(np.ones_like(same), 1)
    lo, hi = s[~same & upper].max(), s[same & upper].min()
    assert lo < 0.7 < 0.85 < hi
    threshold = 0.5 * (float(lo) + float(hi))
    for kw in (dict(threshold=threshold), dict(target=k)):
        labels, first, second, bounds = R2.two_pass(s, first_pass_max_points=cap, **kw)
        assert bounds == R2.subsets(n, cap) and len(first) == len(bounds) - 1 >= 2
        assert labels.tolist() == R.cluster(s, **kw)[0].tolist() == _partition(who)
    # with a target the first pass stops at ten times the target per subset, and the second pass does the rest
    labels, first, second, bounds = R2.two_pass(s, target=1, first_pass_max_points=cap)
    assert [len(m) for m, _ in first] == [max(0, b - a - 10) for a, b in zip(bounds[:-1], bounds[1:])]
    assert len(second[0]) == sum(min(b - a, 10) for a, b in zip(bounds[:-1], bounds[1:])) - 1 and (labels == 0).all()


def test_a_short_recording_is_one_pass():
    s, _ = R.clustered_scores(4, 65, 3)
    for kw in (dict(threshold=0.3), dict(target=3), dict(target=65)):
        labels, first, second, bounds = R2.two_pass(s, first_pass_max_points=65, **kw)
        want = R.cluster(s, **kw)
        assert bounds == [0, 65] and len(second[0]) == 0
        _same((labels, first[0][0], first[0][1]), want)
