"""NumPy restatement of xv_ahc_cluster (include/xvector_hip.h): average-linkage agglomerative clustering on scores, in the arithmetic of
`dtype`.  At float32 every operation is the kernel's - one IEEE add per merged entry, one IEEE divide per average - so the merge log is
the same bits; at float64 it is the reference the decision-stable cases are compared with.  stability() says how far every decision of a
run is from flipping under fp32 rounding."""
import numpy as np


def upper_symmetric(s, dtype):
    """T[i][j] = T[j][i] = s[min(i,j)][max(i,j)], the diagonal zero: what the operation reads of s."""
    u = np.triu(np.asarray(s, dtype=dtype), 1)
    return u + u.T


def cluster(s, threshold=0.0, target=0, dtype=np.float32):
    """-> (labels int32 [n], merges int32 [m, 2], merge_values dtype [m]) of one score matrix s [n, >= n] (columns beyond n are ignored)."""
    s = np.asarray(s)
    n = s.shape[0]
    t = upper_symmetric(s[:, :n], dtype)
    size = np.ones(n, np.int64)
    low = np.array(-np.inf, dtype)
    # A[a][b] for active a < b, -inf elsewhere: argmax over the flattened matrix returns the first largest entry in row-major order -
    # the lowest a, then the lowest b
    avg = np.where(np.triu(np.ones((n, n), bool), 1), t, low).astype(dtype)      # (singletons: T / (float)(1 * 1) is T)
    merges, values = [], []
    count, stop_at = n, max(int(target), 1)
    while count > stop_at:
        a, b = divmod(int(np.argmax(avg)), n)
        v = avg[a, b]
        if target == 0 and not v >= dtype(threshold):
            break
        merges.append((a, b))
        values.append(v)
        others = (size > 0)
        others[[a, b]] = False
        t[a, others] = t[a, others] + t[b, others]
        t[others, a] = t[a, others]
        size[a] += size[b]
        size[b] = 0
        avg[b, :] = low
        avg[:, b] = low
        k = np.nonzero(others)[0]
        new = t[a, k] / (size[a] * size[k]).astype(dtype)
        avg[np.minimum(a, k), np.maximum(a, k)] = new
        count -= 1
    root = np.arange(n)
    for a, b in merges:
        root[root == b] = a
    ids = np.unique(root)
    return (np.searchsorted(ids, root).astype(np.int32), np.asarray(merges, np.int32).reshape(-1, 2), np.asarray(values, dtype))


def partitions(n, merges):
    """The partition after each merge, as a tuple of root ids per item (a cluster's id is its smallest member)."""
    root = np.arange(n)
    out = []
    for a, b in merges:      # a and b are cluster ids: b's members carry root b until now
        root = np.where(root == b, a, root)
        out.append(tuple(root))
    return out


def stability(s, threshold=0.0, target=0):
    """Per step of the float64 run on s: the smallest (A_best - A_c) / (e_best + e_c) over every other active pair c, where
    e = 2^-24 (depth + 1) sum|s| / (size_a size_b) bounds the fp32 error of a pair's average (depth: the longest chain of adds behind its
    T entry, sum|s|: the absolute scores it sums).  A run whose smallest figure is well above 1 takes the same decisions in fp32.
    -> float64 [steps] (inf at a step with a single pair)."""
    s = np.asarray(s, np.float64)
    n = s.shape[0]
    t = upper_symmetric(s[:, :n], np.float64)
    tabs = np.abs(t)
    depth = np.zeros((n, n))
    size = np.ones(n)
    active = np.ones(n, bool)
    out = []
    count, stop_at = n, max(int(target), 1)
    while count > stop_at:
        pair = np.triu(np.outer(active, active), 1)
        prod = np.outer(size, size)
        avg = np.where(pair, t / np.where(pair, prod, 1.0), -np.inf)
        err = np.where(pair, 2.0 ** -24 * (depth + 1.0) * tabs / np.where(pair, prod, 1.0), 0.0)
        a, b = divmod(int(np.argmax(avg)), n)
        if target == 0 and not avg[a, b] >= threshold:
            break
        rest = pair.copy()
        rest[a, b] = False
        with np.errstate(divide="ignore", invalid="ignore"):
            out.append(((avg[a, b] - avg[rest]) / (err[a, b] + err[rest])).min() if rest.any() else np.inf)
        others = active.copy()
        others[[a, b]] = False
        for m in (t, tabs):
            m[a, others] = m[a, others] + m[b, others]
            m[others, a] = m[a, others]
        depth[a, others] = np.maximum(depth[a, others], depth[b, others]) + 1.0
        depth[others, a] = depth[a, others]
        size[a] += size[b]
        active[b] = False
        count -= 1
    return np.asarray(out, np.float64)


def clustered_scores(seed, n, k, dim=16, noise=0.6):
    """The generator the decision-stable cases use: k means randn(k, dim), labels randint(0, k, n), x = mean + noise * randn, unit rows,
    S = x x^T rounded to fp32.  -> (S float32 [n, n], labels)."""
    rs = np.random.RandomState(seed)
    means = rs.randn(k, dim)
    labels = rs.randint(0, k, n)
    x = means[labels] + noise * rs.randn(n, dim)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return (x @ x.T).astype(np.float32), labels
