"""fp64 restatement of PLDA domain adaptation and of AS-norm of PLDA scores, what the tests of
misc/backend.py adapt_plda / Backend.adapt / BackendScorer.cohort and of csrc/xv_backend_cohort.hip compare with.  Kaldi is not available
where the tests run, so this is parity by restatement: the steps of the specification written a second time, in double, with explicit
diagonal matrices and loops where the package uses broadcasting, a full sort where the kernel selects, and the closed-form log-likelihood
ratio of tests/backend_ref.py where the kernel uses its factored form.  It imports nothing of the package's back end.
tests/test_backend_adapt_ref.py holds it against derivations that do not share its code."""
import numpy as np

from tests import backend_ref as R

VAR_FLOOR = 1e-12


def _eigh_desc(m):
    w, v = np.linalg.eigh(0.5 * (m + m.T))
    order = np.argsort(-w, kind="stable")
    return w[order], v[:, order]


def adapt_stats(y):
    """(mean, sum y y^T, n) of the adaptation vectors y, rows in double, by a loop."""
    y = np.asarray(y, dtype=np.float64)
    acc, s = np.zeros(y.shape[1]), np.zeros((y.shape[1], y.shape[1]))
    for row in y:
        acc += row
        s += np.outer(row, row)
    return acc / y.shape[0], s, y.shape[0]


def adapt(model, mean_y, scatter_y, n, within=0.3, between=0.7, mean_diff=1.0):
    """PldaUnsupervisedAdaptor::UpdatePlda, step by step as INTEGRATION.md section 6b numbers them.  model: dict(mean, transform, psi).
    -> dict(mean, transform, psi, offset, s): s the eigenvalues of step 2, descending."""
    mean, t, psi = np.asarray(model["mean"], np.float64), np.asarray(model["transform"], np.float64), np.asarray(model["psi"], np.float64)
    d = psi.shape[0]
    m = np.asarray(mean_y, np.float64)
    # 1
    v = np.asarray(scatter_y, np.float64) / n - np.outer(m, m) + mean_diff * np.outer(m - mean, m - mean)
    # 2
    mm = np.diag(1.0 / np.sqrt(1.0 + psi)) @ t
    s, p = _eigh_desc(mm @ v @ mm.T)
    # 3
    w2 = p.T @ np.diag(1.0 / (1.0 + psi)) @ p
    b2 = p.T @ np.diag(psi / (1.0 + psi)) @ p
    for i in range(d):
        if s[i] > 1.0:
            w2[i, i] += within * (s[i] - 1.0)
            b2[i, i] += between * (s[i] - 1.0)
    # 4
    k = np.linalg.inv(p.T @ mm)
    wm, bm = k @ w2 @ k.T, k @ b2 @ k.T
    # 5
    c1 = np.linalg.inv(np.linalg.cholesky(0.5 * (wm + wm.T)))
    psi_new, q = _eigh_desc(c1 @ bm @ c1.T)
    psi_new = np.maximum(psi_new, 0.0)
    transform = q.T @ c1
    return dict(mean=m, transform=transform, psi=psi_new, offset=-(transform @ m), s=s)


def total_covariance(model):
    """T^-1 (I + diag psi) T^-T: the covariance the model gives a single vector."""
    ti = np.linalg.inv(np.asarray(model["transform"], np.float64))
    return ti @ np.diag(1.0 + np.asarray(model["psi"], np.float64)) @ ti.T


def dense_llr(e, t, psi, n_utts=None):
    """[rows of e, rows of t]: LLR(e_r, t_j), e_r a model of n_utts[r] utterances, by backend_ref.llr_trials (the closed form)."""
    e, t = np.asarray(e, np.float64), np.asarray(t, np.float64)
    n = np.ones(e.shape[0]) if n_utts is None else np.asarray(n_utts)
    ti = np.arange(t.shape[0])
    return np.stack([R.llr_trials(e[r:r + 1], t, np.zeros_like(ti), ti, psi, n[r:r + 1]) for r in range(e.shape[0])])      # a row at a time


def top_k_stats(scores, top_k):
    """[rows, 2]: mean and biased deviation sqrt(max(var, 1e-12)) of each row's min(top_k, n) largest scores (full sort)."""
    scores = np.asarray(scores, np.float64)
    k = min(int(top_k), scores.shape[1])
    out = np.zeros((scores.shape[0], 2))
    for r, row in enumerate(scores):
        top = np.sort(row)[::-1][:k]
        mu = top.sum() / k
        out[r] = mu, np.sqrt(max(((top - mu) ** 2).sum() / k, VAR_FLOOR))
    return out


def as_norm(e, t, c, ei, ti, psi, top_k, enrol_n=None):
    """AS-normed PLDA scores of trials: e prepared with its counts enrol_n, t and the cohort c with one utterance.  The model side's
    statistics use the model's count, the test side's treat the test vector as a one-utterance model.  -> (scores, raw, e_stats, t_stats)."""
    raw = R.llr_trials(e, t, ei, ti, psi, enrol_n)
    e_stats = top_k_stats(dense_llr(e, c, psi, enrol_n), top_k)
    t_stats = top_k_stats(dense_llr(t, c, psi), top_k)
    ei, ti = np.asarray(ei), np.asarray(ti)
    return 0.5 * ((raw - e_stats[ei, 0]) / e_stats[ei, 1] + (raw - t_stats[ti, 0]) / t_stats[ti, 1]), raw, e_stats, t_stats


def prepared(mean, lda_mat, plda, x, n_utts=None):
    """Raw fp32 rows through the whole chain (centre, LDA, length normalisation, PLDA transform and normalisation), in double."""
    u = R.unit_chain(mean, lda_mat, x)
    model = dict(plda, offset=-(np.asarray(plda["transform"]) @ np.asarray(plda["mean"])))
    return R.plda_transform(model, u * np.sqrt(float(u.shape[1])), n_utts)


def adapt_backend(mean_old, lda_mat, plda, x_adapt, within=0.3, between=0.7, mean_diff=1.0, perturb=None):
    """Backend.adapt on exact fp64 statistics: -> (new mean fp32, adapted model).  perturb(scatter, sum of |products|) -> scatter, optional:
    the sensitivity runs of the end-to-end test."""
    mean_new = R.global_mean(x_adapt)
    y = R.unit_chain(mean_new, lda_mat, x_adapt) * np.sqrt(float(plda["psi"].shape[0]))
    m, s, n = adapt_stats(y)
    if perturb is not None:
        s = perturb(s, R.scatter_abs(y))
    return mean_new, adapt(plda, m, s, n, within, between, mean_diff)
