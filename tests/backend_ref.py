"""fp64 restatement of the LDA / PLDA back end, what the tests of misc/backend.py and csrc/xv_backend.hip compare
with.  Kaldi is not available where the tests run, so this is parity by restatement: the arithmetic of the specification written a second
time, in double, with straight loops over speakers and utterances where the package uses statistics and groups.  It reads the same fp32
inputs and imports nothing of the package's back end.  tests/test_backend_ref.py holds it against derivations that do not share its code."""
import numpy as np


def chain(d):
    """Longest add chain of a row sum of the one-wave-per-row kernels (stated in csrc/xv_rowsum.h)."""
    return 4 * ((d + 255) // 256) + 6


def global_mean(x):
    """ivector-mean: column sums in fp64, the mean rounded to fp32."""
    x = np.asarray(x, dtype=np.float64)
    acc = np.zeros(x.shape[1])
    for row in x:
        acc += row
    return (acc / x.shape[0]).astype(np.float32)


def group_means(x, d, offsets, rows):
    """Sequential fp64 sum of each group's rows in list order, one divide."""
    out = np.zeros((len(offsets) - 1, d), np.float64)
    for g in range(len(offsets) - 1):
        acc = np.zeros(d, np.float64)
        for i in range(int(offsets[g]), int(offsets[g + 1])):
            acc = acc + x[int(rows[i]), :d].astype(np.float64)
        out[g] = acc / np.float64(int(offsets[g + 1]) - int(offsets[g]))
    return out


def center(x, mean):
    """fp32(x - mean): the subtraction is done in fp32, as the device does it; returned in double."""
    x = np.asarray(x, dtype=np.float32)
    return (x if mean is None else x - np.asarray(mean, dtype=np.float32)).astype(np.float64)


def scatter(v):
    v = np.asarray(v, dtype=np.float64)
    return v.T @ v


def scatter_abs(v):
    """sum_r |v_ri v_rj|: what the scatter tolerance is relative to."""
    a = np.abs(np.asarray(v, dtype=np.float64))
    return a.T @ a


def length_norm(z):
    """ivector-normalize-length, scale-up on: norm sqrt(dim)."""
    z = np.asarray(z, dtype=np.float64)
    n = np.sqrt((z * z).sum(axis=1, keepdims=True))
    return z * np.sqrt(float(z.shape[1])) / np.where(n > 0, n, 1.0)


def lda(v, groups, dim, f=0.0, floor=1e-6):
    """ivector-compute-lda on centred vectors v (double), groups = list of row-index lists.  -> ([dim, d + 1], l descending, floor active)."""
    v = np.asarray(v, dtype=np.float64)
    d = v.shape[1]
    tot, btw, n_all, mu = np.zeros((d, d)), np.zeros((d, d)), 0, np.zeros(d)
    for idx in groups:
        m = np.zeros(d)
        for i in idx:
            tot += np.outer(v[i], v[i])
            m += v[i]
            mu += v[i]
        m /= len(idx)
        btw += len(idx) * np.outer(m, m)
        n_all += len(idx)
    total, within = tot / n_all, (tot - btw) / n_all
    s, u = np.linalg.eigh(f * total + (1.0 - f) * within)
    active = bool(s.min() < s.max() * floor)
    s = np.maximum(s, s.max() * floor)
    t = np.diag(s ** -0.5) @ u.T
    bp = t @ (total - within) @ t.T
    l, vv = np.linalg.eigh(0.5 * (bp + bp.T))
    order = np.argsort(-l, kind="stable")
    l, vv = l[order], vv[:, order]
    a = vv[:, :dim].T @ t
    return np.concatenate([a, -(a @ (mu / n_all))[:, None]], axis=1), l, active, total, within


def transform_vec(mat, v):
    """transform-vec with a d + 1 column matrix: A v + b."""
    mat = np.asarray(mat, dtype=np.float64)
    return np.asarray(v, dtype=np.float64) @ mat[:, :-1].T + mat[:, -1]


def plda_stats(y, groups):
    """(S, per-speaker means, counts) by a loop over the speakers."""
    y = np.asarray(y, dtype=np.float64)
    d = y.shape[1]
    s, means, counts = np.zeros((d, d)), [], []
    for idx in groups:
        ys = y[list(idx)]
        m = ys.sum(axis=0) / len(idx)
        s += ys.T @ ys - len(idx) * np.outer(m, m)
        means.append(m)
        counts.append(len(idx))
    return s, np.asarray(means), np.asarray(counts)


def plda_em(s, means, counts, iters=10):
    """ivector-compute-plda from S and the per-speaker means, one speaker at a time."""
    k, d = means.shape
    mu = means.sum(axis=0) / k
    w, b = np.eye(d), np.eye(d)
    for _ in range(iters):
        wst, wc, bst, bc = s.copy(), float(counts.sum() - k), np.zeros((d, d)), 0.0
        w_inv, b_inv = np.linalg.inv(w), np.linalg.inv(b)
        for sp in range(k):
            n = float(counts[sp])
            mn = np.linalg.inv(b_inv + n * w_inv)
            m = means[sp] - mu
            ww = mn @ (n * (w_inv @ m))
            bst += mn + np.outer(ww, ww)
            bc += 1
            wst += n * mn + n * np.outer(m - ww, m - ww)
            wc += 1
        w, b = wst / wc, bst / bc
    lo = np.linalg.cholesky(0.5 * (w + w.T))
    t1 = np.linalg.inv(lo)
    bb = t1 @ b @ t1.T
    psi, u = np.linalg.eigh(0.5 * (bb + bb.T))
    order = np.argsort(-psi, kind="stable")
    psi, u = np.maximum(psi[order], 0.0), u[:, order]
    transform = u.T @ t1
    return dict(mean=mu, transform=transform, psi=psi, offset=-(transform @ mu), within=w, between=b)


def plda_normalize(u, psi, n_utts=None):
    u, psi = np.asarray(u, dtype=np.float64), np.asarray(psi, dtype=np.float64)
    n = np.ones(u.shape[0]) if n_utts is None else np.asarray(n_utts, dtype=np.float64)
    s = (u * u / (psi[None, :] + 1.0 / n[:, None])).sum(axis=1, keepdims=True)
    return u * np.sqrt(u.shape[1] / np.where(s > 0, s, 1.0)) * (s > 0)


def plda_transform(model, y, n_utts=None):
    """Plda::TransformIvector with normalize_length: offset + transform y, then the PLDA normalisation."""
    u = np.asarray(y, dtype=np.float64) @ model["transform"].T + model["offset"]
    return plda_normalize(u, model["psi"], n_utts)


def llr(e, t, psi, n):
    """Plda::LogLikelihoodRatio for one trial: enrol e with n utterances against test t."""
    psi = np.asarray(psi, dtype=np.float64)
    total = 0.0
    for c in range(psi.shape[0]):
        a = n * psi[c] / (n * psi[c] + 1.0)
        v = 1.0 + psi[c] / (n * psi[c] + 1.0)
        total += -0.5 * (np.log(v) + (t[c] - a * e[c]) ** 2 / v) + 0.5 * (np.log(psi[c] + 1.0) + t[c] ** 2 / (psi[c] + 1.0))
    return total


def llr_trials(e, t, ei, ti, psi, n_utts=None):
    e, t = np.asarray(e, dtype=np.float64), np.asarray(t, dtype=np.float64)
    psi = np.asarray(psi, dtype=np.float64)[None, :]
    n = (np.ones(e.shape[0]) if n_utts is None else np.asarray(n_utts, dtype=np.float64))[np.asarray(ei)][:, None]
    a, v = n * psi / (n * psi + 1.0), 1.0 + psi / (n * psi + 1.0)
    ee, tt = e[np.asarray(ei)], t[np.asarray(ti)]
    return (-0.5 * (np.log(v) + (tt - a * ee) ** 2 / v) + 0.5 * (np.log(psi + 1.0) + tt * tt / (psi + 1.0))).sum(axis=1)


def coefficients(psi, distinct_n):
    """(a, iv, g, k0) in double for each distinct n, element by element."""
    psi = np.asarray(psi, dtype=np.float64)
    a, iv, k0 = [], [], []
    for n in distinct_n:
        n = float(n)
        a.append([n * p / (n * p + 1.0) for p in psi])
        iv.append([1.0 / (1.0 + p / (n * p + 1.0)) for p in psi])
        k0.append(sum(-0.5 * np.log(1.0 + p / (n * p + 1.0)) + 0.5 * np.log(p + 1.0) for p in psi))
    return np.asarray(a), np.asarray(iv), np.asarray([1.0 / (p + 1.0) for p in psi]), np.asarray(k0)


def trials_from_tables(e, t, ei, ti, nidx, coef, g, k0, d):
    """The sum xv_backend_plda_trials computes, from the SAME fp32 tables, in double: (scores, sum of the |terms|)."""
    e, t = np.asarray(e, dtype=np.float64)[:, :d], np.asarray(t, dtype=np.float64)[:, :d]
    coef, g, k0 = np.asarray(coef, dtype=np.float64), np.asarray(g, dtype=np.float64)[:d], np.asarray(k0, dtype=np.float64)
    q = np.asarray(nidx)[np.asarray(ei)]
    ee, tt = e[np.asarray(ei)], t[np.asarray(ti)]
    t1 = -0.5 * coef[q, 1, :d] * (tt - coef[q, 0, :d] * ee) ** 2
    t2 = 0.5 * g[None, :] * tt * tt
    return k0[q] + (t1 + t2).sum(axis=1), (np.abs(t1) + np.abs(t2)).sum(axis=1), k0[q]


def unit_chain(backend_mean, lda_mat, x):
    """centre -> LDA (None: none) -> unit length, rows in double."""
    v = center(x, backend_mean)
    z = v if lda_mat is None else transform_vec(lda_mat, v)
    n = np.sqrt((z * z).sum(axis=1, keepdims=True))
    return z / np.where(n > 0, n, 1.0)


def train(x, groups, lda_dim, iters=10, perturb=None):
    """The whole training on fp32 inputs x with exact fp64 statistics: -> (mean fp32, lda [dim, d + 1] or None, plda dict).
    perturb(name, matrix, sum of |products|) -> matrix, optional: applied to the two scatter statistics (the sensitivity runs of the end-to-end test)."""
    mean = global_mean(x)
    v = center(x, mean)
    lda_mat = None
    if lda_dim:
        d = v.shape[1]
        used = [i for idx in groups for i in idx]
        tot = scatter(v[used])
        if perturb is not None:
            tot = perturb("lda", tot, scatter_abs(v[used]))
        means = np.asarray([v[list(idx)].sum(axis=0) / len(idx) for idx in groups])
        counts = np.asarray([len(idx) for idx in groups], dtype=np.float64)
        n = counts.sum()
        btw = (means * counts[:, None]).T @ means
        total, within = tot / n, (tot - btw) / n
        s, u = np.linalg.eigh(within)
        s = np.maximum(s, s.max() * 1e-6)
        t = np.diag(s ** -0.5) @ u.T
        bp = t @ (total - within) @ t.T
        l, vv = np.linalg.eigh(0.5 * (bp + bp.T))
        vv = vv[:, np.argsort(-l, kind="stable")]
        a = vv[:, :lda_dim].T @ t
        lda_mat = np.concatenate([a, -(a @ (counts @ means / n))[:, None]], axis=1).astype(np.float32)      # transform.mat is a float matrix
    y = unit_chain(mean, lda_mat, x) * np.sqrt(float(lda_dim or x.shape[1]))
    used = [i for idx in groups for i in idx]
    tot_y = scatter(y[used])
    if perturb is not None:
        tot_y = perturb("plda", tot_y, scatter_abs(y[used]))
    means = np.asarray([y[list(idx)].sum(axis=0) / len(idx) for idx in groups])
    counts = np.asarray([len(idx) for idx in groups])
    s = tot_y - (means * counts[:, None]).T @ means
    return mean, lda_mat, plda_em(0.5 * (s + s.T), means, counts, iters)


def score(mean, lda_mat, plda, enrol, test, ei, ti, mode, enrol_n=None):
    """Scores of raw fp32 tables through the chain, in double: "lda_cos" or "plda"."""
    e, t = unit_chain(mean, lda_mat, enrol), unit_chain(mean, lda_mat, test)
    if mode == "lda_cos":
        return (e[np.asarray(ei)] * t[np.asarray(ti)]).sum(axis=1)
    dim = e.shape[1]
    eu = plda_transform(plda, e * np.sqrt(float(dim)), enrol_n)
    tu = plda_transform(plda, t * np.sqrt(float(dim)))
    return llr_trials(eu, tu, ei, ti, plda["psi"], enrol_n)


def eer(scores, targets):
    """Equal error rate by a threshold sweep over the sorted scores (no SciPy): the point where miss and false-alarm rates cross."""
    scores, targets = np.asarray(scores, dtype=np.float64), np.asarray(targets).astype(bool)
    order = np.argsort(-scores, kind="stable")
    t = targets[order]
    tp, fp = np.cumsum(t), np.cumsum(~t)
    miss, fa = 1.0 - tp / t.sum(), fp / (~t).sum()
    i = int(np.argmin(np.abs(miss - fa)))
    return 0.5 * (miss[i] + fa[i])
