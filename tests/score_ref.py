"""fp64 NumPy restatement of the scoring ops (csrc/xv_score.hip, include/xvector_hip.h) and of AS-norm, what the GPU tests compare with.
Kaldi is not available where the tests run, so this is parity by restatement: the arithmetic of the header written a second time, in
double, with a full sort where the kernel selects.  tests/test_score_ref.py holds it against literal per-element loops."""
import numpy as np

EPS = 1e-12


def chain(d):
    """Longest add chain of a row sum of the prepare / trial kernels (stated in xv_score.hip and the header)."""
    return 4 * ((d + 255) // 256) + 6


def prepare(x, d=None, mean=None):
    """[rows, d]: (x[:, :d] - mean) scaled by 1 / sqrt(max(sum of squares, 1e-12))."""
    x = np.asarray(x, dtype=np.float64)
    d = x.shape[1] if d is None else d
    v = x[:, :d] - (0.0 if mean is None else np.asarray(mean, dtype=np.float64)[:d])
    return v / np.sqrt(np.maximum((v * v).sum(axis=1, keepdims=True), EPS))


def trials(e, t, ei, ti, e_stats=None, t_stats=None):
    e, t = np.asarray(e, dtype=np.float64), np.asarray(t, dtype=np.float64)
    s = (e[ei] * t[ti]).sum(axis=1)
    if e_stats is None and t_stats is None:
        return s
    e_stats, t_stats = np.asarray(e_stats, dtype=np.float64), np.asarray(t_stats, dtype=np.float64)
    return 0.5 * ((s - e_stats[ei, 0]) / e_stats[ei, 1] + (s - t_stats[ti, 0]) / t_stats[ti, 1])


def cohort_scores(x, cohort):
    return np.asarray(x, dtype=np.float64) @ np.asarray(cohort, dtype=np.float64).T


def top_k_stats(scores, top_k):
    """[rows, 2]: mean and biased deviation sqrt(max(var, 1e-12)) of each row's min(top_k, n) largest scores (full sort)."""
    scores = np.asarray(scores, dtype=np.float64)
    k = min(int(top_k), scores.shape[1])
    top = -np.sort(-scores, axis=1)[:, :k]
    mean = top.mean(axis=1)
    var = ((top - mean[:, None]) ** 2).mean(axis=1)
    return np.stack([mean, np.sqrt(np.maximum(var, EPS))], axis=1)


def cohort_stats(x, cohort, top_k):
    return top_k_stats(cohort_scores(x, cohort), top_k)


def score_pipeline(enrol, test, ei, ti, center=None, cohort=None, top_k=0):
    """What nnet/lib/score.py computes from raw tables: centre (the given mean), length-normalise, dot, AS-norm with the cohort."""
    e, t = prepare(enrol, mean=center), prepare(test, mean=center)
    if cohort is None:
        return trials(e, t, ei, ti)
    c = prepare(cohort, mean=center)
    return trials(e, t, ei, ti, cohort_stats(e, c, top_k), cohort_stats(t, c, top_k))
