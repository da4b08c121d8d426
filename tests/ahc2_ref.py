"""NumPy restatement of the two-pass clustering of long recordings (include/xvector_hip.h): xv_ahc_cluster_from - the clusterer of
tests/ahc_ref.py with a floor, a threshold and a seeded start -, xv_ahc_cluster_sums - the seed of the second pass, every sum in the
stated order -, and the driver ops.ahc_cluster_two_pass.  At float32 every operation is the kernels', so merge logs, labels and seeds
are the same bits.  The sums are sequential: np.cumsum adds one term after the other (np.sum adds pairwise and is not used)."""
import numpy as np

from tests import ahc_ref as R

MAX_CLUSTERS = 2048      # what the second pass takes


def cluster_from(t, sizes, floor=1, threshold=-np.inf, dtype=np.float32):
    """The seeded clusterer: c clusters of `sizes` (each >= 1) and their sums t [c, c] (symmetric; the diagonal is not read).  Merging goes
    on while count > floor and the best A >= threshold.  A = t[a][b] / dtype(size_a * size_b): the integer product is converted once, round
    to nearest even.  -> (labels int32 [c], merges int32 [m, 2], merge_values dtype [m]), numbered as tests/ahc_ref.py numbers them."""
    t = np.array(t, dtype=dtype)
    c = t.shape[0]
    size = np.array(sizes, np.int64)
    assert size.shape == (c,) and (size >= 1).all() and 1 <= floor
    low = np.array(-np.inf, dtype)
    upper = np.triu(np.ones((c, c), bool), 1)
    prod = np.where(upper, np.outer(size, size), 1).astype(dtype)
    avg = np.where(upper, t / prod, low).astype(dtype)
    merges, values = [], []
    count = c
    while count > floor:
        a, b = divmod(int(np.argmax(avg)), c)      # the first largest entry in row-major order: the lowest a, then the lowest b
        v = avg[a, b]
        if not v >= dtype(threshold):
            break
        merges.append((a, b))
        values.append(v)
        others = size > 0
        others[[a, b]] = False
        t[a, others] = t[a, others] + t[b, others]
        t[others, a] = t[a, others]
        size[a] += size[b]
        size[b] = 0
        avg[b, :] = low
        avg[:, b] = low
        k = np.nonzero(others)[0]
        avg[np.minimum(a, k), np.maximum(a, k)] = t[a, k] / (size[a] * size[k]).astype(dtype)
        count -= 1
    root = np.arange(c)
    for a, b in merges:
        root[root == b] = a
    ids = np.unique(root)
    return (np.searchsorted(ids, root).astype(np.int32), np.asarray(merges, np.int32).reshape(-1, 2), np.asarray(values, dtype))


def cluster_from_scores(s, floor=1, threshold=-np.inf, dtype=np.float32):
    """The start from scores: singletons, t from the upper triangle of s [n, >= n]."""
    n = np.asarray(s).shape[0]
    return cluster_from(R.upper_symmetric(np.asarray(s)[:, :n], dtype), np.ones(n, np.int64), floor, threshold, dtype)


def member_lists(labels):
    """Labels 0, 1, ... numbered by smallest member -> [members of cluster 0 ascending, of cluster 1, ...]."""
    labels = np.asarray(labels)
    return [np.flatnonzero(labels == k) for k in range(int(labels.max()) + 1)]


def cluster_sums(s, lists):
    """The seed: for clusters A < B, r_i[B] = the sequential double sum over j in B ascending of e(i, j) = s[min(i,j)][max(i,j)],
    T[A][B] = T[B][A] = float32(the sequential double sum over i in A ascending of r_i[B]); the diagonal is 0.  -> (T float32 [c, c],
    sizes int32 [c])."""
    n = np.asarray(s).shape[0]
    e = R.upper_symmetric(np.asarray(s)[:, :n], np.float64)      # (the diagonal is 0: the term j = i of a row's own cluster, never used)
    c = len(lists)
    rows = np.empty((n, c), np.float64)
    for b, members in enumerate(lists):
        rows[:, b] = np.cumsum(e[:, members], axis=1)[:, -1]
    t = np.zeros((c, c), np.float32)
    for a, members in enumerate(lists):
        line = np.cumsum(rows[members, :], axis=0)[-1].astype(np.float32)
        t[a, a + 1:] = line[a + 1:]
        t[a + 1:, a] = line[a + 1:]
    return t, np.asarray([len(m) for m in lists], np.int32)


def subsets(n, first_pass_max_points):
    """The boundaries of the first pass's contiguous subsets: ceil(n / first_pass_max_points) of them, ceil(n / that number) rows each."""
    count = -(-n // first_pass_max_points)
    size = -(-n // count)
    return [min(k * size, n) for k in range(count + 1)]


def two_pass(s, threshold=0.0, target=0, first_pass_max_points=2048, dtype=np.float32):
    """ops.ahc_cluster_two_pass on one recording: target 0 = by threshold.  -> (labels int32 [n], [first-pass (merges, values) per subset],
    second-pass (merges, values), the subset boundaries)."""
    s = np.asarray(s)
    n = s.shape[0]
    end = max(int(target), 1)
    stop = threshold if target == 0 else -np.inf
    bounds = subsets(n, first_pass_max_points)
    clusters, c, first = np.empty(n, np.int64), 0, []
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        floor = min(hi - lo, 10 * end) if len(bounds) > 2 else end
        labels, merges, values = cluster_from_scores(s[lo:hi, lo:hi], floor, stop, dtype)
        first.append((merges, values))
        clusters[lo:hi] = c + labels
        c += int(labels.max()) + 1
    if c > MAX_CLUSTERS:
        raise ValueError("the first pass leaves %d clusters" % c)
    t, sizes = cluster_sums(s, member_lists(clusters))
    labels, merges, values = cluster_from(t, sizes, end if len(bounds) > 2 else c, stop, dtype)
    return labels[clusters], first, (merges, values), bounds
