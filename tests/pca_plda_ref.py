"""fp64 NumPy restatement of xv_backend_pca_plda (include/xvector_hip.h states the arithmetic): the per-recording PCA of Kaldi's
ivector-plda-scoring-dense --target-energy as this project recalls it - nothing here is compared with a run of Kaldi -, the PLDA model
projected into the kept subspace and diagonalised again, with numpy.linalg.eigh / cholesky where the device runs its Jacobi and its own
Cholesky.  Also the scores that follow (affine map -> PLDA normalisation -> one-utterance log-likelihood ratios), the decision-gap check
that says when a comparison of p and of scores with another implementation is meaningful, and the four-speaker case generator the tests
share."""
import numpy as np

from tests import backend_ref as R


def covariances(plda):
    """(W, B): the within- and between-class covariances of a PLDA model (mean, transform T, psi): W = T^-1 T^-T, B = T^-1 diag(psi) T^-T,
    symmetrised."""
    ti = np.linalg.inv(np.asarray(plda["transform"], dtype=np.float64))
    w, b = ti @ ti.T, (ti * np.asarray(plda["psi"], dtype=np.float64)[None, :]) @ ti.T
    return 0.5 * (w + w.T), 0.5 * (b + b.T)


def _eigh_desc(m):
    w, v = np.linalg.eigh(0.5 * (m + m.T))
    order = np.argsort(-w, kind="stable")
    return w[order], v[:, order]


def covariance(x):
    """C = (1 / n) sum x x^T - m m^T of the fp32 rows x, in double."""
    x = np.asarray(x, dtype=np.float64)
    m = x.mean(axis=0)
    return x.T @ x / x.shape[0] - np.outer(m, m)


def energy_dim(s, target):
    """Kaldi's loop: dim = 1, e = 0; while e / sum s <= target: e += s[dim - 1]; dim++ - capped at len(s)."""
    total, e, dim = float(np.sum(s)), 0.0, 1
    while dim <= len(s) and e / total <= target:
        e += float(s[dim - 1])
        dim += 1
    return min(dim, len(s))


def estimate(x, w, b, mu, target, basis=None):
    """The per-recording model of the unit-length fp32 rows x [n, D] -> dict(p, s, q, psi, tp, a, offset), all double; p = 0 (and only p and
    s) for n = 1 or a zero covariance.  a = sqrt(D) T' Q and offset = -T' Q mu map a unit-length row into the space where W' is I and B'
    diag(psi).  basis: an orthogonal [p, p] matrix R that replaces Q by R Q (the scores must not depend on it)."""
    x = np.asarray(x, dtype=np.float64)
    n, d = x.shape
    s, pm = _eigh_desc(covariance(x))
    s = np.maximum(s, 0.0)
    if n == 1 or not s.sum() > 0.0:
        return dict(p=0, s=s)
    p = energy_dim(s, target)
    q = pm[:, :p].T
    if basis is not None:
        q = np.asarray(basis, dtype=np.float64) @ q
    wp, bp = q @ w @ q.T, q @ b @ q.T
    wp, bp = 0.5 * (wp + wp.T), 0.5 * (bp + bp.T)
    t1 = np.linalg.inv(np.linalg.cholesky(wp))
    psi, u = _eigh_desc(t1 @ bp @ t1.T)
    psi = np.maximum(psi, 0.0)
    tp = u.T @ t1
    return dict(p=p, s=s, q=q, psi=psi, tp=tp, wp=wp, bp=bp, a=np.sqrt(float(d)) * (tp @ q), offset=-(tp @ (q @ np.asarray(mu, dtype=np.float64))))


def scores_from(x, a, offset, psi):
    """The [n, n] one-utterance log-likelihood ratios of the rows x behind the map (a, offset) and the PLDA normalisation with psi, double."""
    u = np.asarray(x, dtype=np.float64) @ np.asarray(a, dtype=np.float64).T + np.asarray(offset, dtype=np.float64)
    y = R.plda_normalize(u, psi)
    n = y.shape[0]
    ei, ti = (g.reshape(-1) for g in np.meshgrid(np.arange(n), np.arange(n), indexing="ij"))
    return R.llr_trials(y, y, ei, ti, psi).reshape(n, n)


def scores(x, w, b, mu, target, basis=None):
    m = estimate(x, w, b, mu, target, basis)
    return None if m["p"] == 0 else scores_from(x, m["a"], m["offset"], m["psi"])


def decision_gaps(x, target):
    """What decides p and the kept subspace, and by how much: (energy gap = min_k |E_k / E - target|, eigenvalue gap (s_p - s_{p+1}) / s_1
    (inf for p = D), p, rank of C)."""
    x = np.asarray(x, dtype=np.float64)
    s = np.maximum(_eigh_desc(covariance(x))[0], 0.0)
    p = energy_dim(s, target)
    rank = int(np.linalg.matrix_rank(x - x.mean(axis=0)))
    egap = float(np.abs(np.cumsum(s) / s.sum() - target).min())
    sgap = float("inf") if p >= len(s) else float((s[p - 1] - s[p]) / s[0])
    return egap, sgap, p, rank


def qualifies(x, target):
    """The decision-gap conditions under which another implementation in double must agree on p and, to rounding, on the scores."""
    egap, sgap, p, rank = decision_gaps(x, target)
    return egap >= 1e-9 and sgap >= 1e-6 and p <= rank


def model(seed, d):
    """A PLDA model on d dimensions at ivector-normalize-length's scale sqrt(d): dict(mean, transform, psi)."""
    rs = np.random.RandomState(1000 + seed)
    transform = np.linalg.qr(rs.randn(d, d))[0] * rs.uniform(1.0, 2.0, d)[None, :] + 0.05 * rs.randn(d, d)
    return dict(mean=0.1 * rs.randn(d), transform=transform, psi=np.sort(rs.uniform(0.05, 5.0, d))[::-1].copy())


def recording(seed, d, n, speakers=4, noise=0.5):
    """n unit-length fp32 rows in d dimensions around `speakers` centres: the windows of one recording."""
    rs = np.random.RandomState(seed)
    spk = rs.randn(speakers, d)
    x = spk[rs.randint(0, speakers, n)] + noise * rs.randn(n, d)
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


# (D, n, targets): the shapes the tests share; seed 0 of `recording` meets the decision-gap conditions at each of them on the reference
# alone (tests/test_pca_plda_ref.py asserts it).  (4, 3) and (5, 3) have rank 2: a target of 0.9 would ask for a third direction.
SHAPES = ((4, 3, (0.1, 0.5)), (5, 3, (0.1, 0.5)), (36, 40, (0.1, 0.5, 0.9)), (130, 129, (0.1, 0.5, 0.9)), (200, 64, (0.1, 0.5, 0.9)))
BIG = (256, 2048, 0.9)      # both caps, once

_CASES = {}


def case(d, n, seed=0):
    """dict(x fp32 [n, d], plda, w, b, mu) of a shape, built once and read only."""
    key = (d, n, seed)
    if key not in _CASES:
        plda = model(0, d)
        w, b = covariances(plda)
        c = dict(x=recording(seed, d, n), plda=plda, w=w, b=b, mu=plda["mean"].copy())
        for v in (c["x"], w, b, c["mu"]):
            v.setflags(write=False)
        _CASES[key] = c
    return _CASES[key]
