"""The LDA / PLDA back end behind extraction (nnet/lib/train_backend.py, nnet/lib/adapt_backend.py, nnet/lib/score.py --backend), with
multi-utterance enrolment, unsupervised domain adaptation and AS-norm of the PLDA scores.

What the reference recipes go to Kaldi for (egs/voxceleb/v1/run.sh:370-401, egs/sre/v1/run.sh:397-492): ivector-mean, ivector-compute-lda,
ivector-compute-plda, ivector-adapt-plda, ivector-subtract-global-mean | transform-vec | ivector-normalize-length, ivector-plda-scoring.  INTEGRATION.md
section 6b is the specification (parity by restatement: nothing compared with a Kaldi run).  Host side: spk2utt files, the CSR form of
groups of keys, the three estimators and the coefficient table of the log-likelihood ratio, all fp64 NumPy on matrices of d x d or smaller.
Device side: Backend.train and Backend.adapt run the statistics that grow with the corpus (per-speaker means, scatter matrices, the
transform chain) through csrc/xv_backend.hip and the project's GEMMs; BackendScorer keeps prepared tables on the GPU as CosineScorer does,
the cohort of AS-norm among them (csrc/xv_backend_cohort.hip).
Not here: DET plots.
"""
import logging
import os

import numpy as np

try:
    from .._host import cat, device_ops, pack_rows, pitch4, steps, upload
    from .scoring import DEFAULT_WORKSPACE_BYTES, center_mean
except (ImportError, ValueError):
    from _host import cat, device_ops, pack_rows, pitch4, steps, upload
    from misc.scoring import DEFAULT_WORKSPACE_BYTES, center_mean

_LOG = logging.getLogger("tf_kaldi_speaker_amd")
PREPARE_ROWS = 1 << 17      # rows per pass of the transform chain: keeps every GEMM operand far below its 4 GB limit


def _kaldi_io():
    try:
        from ..dataset import kaldi_io
    except (ImportError, ValueError):
        from dataset import kaldi_io
    return kaldi_io


def read_spk2utt(path):
    """Kaldi spk2utt lines `speaker utt1 utt2 ...` -> list of (speaker, [utterances]) in file order.  Blank lines are skipped; a speaker
    without an utterance, or named twice, is refused with its line number."""
    out, seen = [], set()
    with open(path, "r") as f:
        for no, line in enumerate(f, 1):
            cols = line.split()
            if not cols:
                continue
            if len(cols) < 2:
                raise ValueError("%s:%d: speaker %s lists no utterance" % (path, no, cols[0]))
            if cols[0] in seen:
                raise ValueError("%s:%d: speaker %s is listed twice" % (path, no, cols[0]))
            seen.add(cols[0])
            out.append((cols[0], cols[1:]))
    return out


class GroupIndex(object):
    """Groups of keys (a spk2utt) against a table's keys, in the CSR form of xv_backend_group_means: names[g] lists the table rows
    rows[offsets[g]:offsets[g + 1]], counts[g] of them.  An utterance without a vector is logged and skipped; a speaker none of whose
    utterances has a vector is logged and dropped."""

    def __init__(self, keys, spk2utt, log=None):
        log = log or _LOG
        at = {k: i for i, k in enumerate(keys)}
        self.names, rows, offsets = [], [], [0]
        self.skipped_utts, self.dropped = 0, []
        for spk, utts in spk2utt:
            found = []
            for u in utts:
                i = at.get(u)
                if i is None:
                    log.info("[INFO] Utterance %s of speaker %s: no vector, skip." % (u, spk))
                    self.skipped_utts += 1
                else:
                    found.append(i)
            if not found:
                log.info("[INFO] Speaker %s: no vector for any utterance, dropped." % spk)
                self.dropped.append(spk)
                continue
            self.names.append(spk)
            rows.extend(found)
            offsets.append(len(rows))
        self.rows = np.asarray(rows, dtype=np.int32)
        self.offsets = np.asarray(offsets, dtype=np.int64)
        self.counts = np.diff(self.offsets)

    def __len__(self):
        return len(self.names)


def _sym_eigh_desc(m):
    w, v = np.linalg.eigh(0.5 * (m + m.T))
    order = np.argsort(-w, kind="stable")
    return w[order], v[:, order]


def estimate_lda(tot, btw_means, counts, dim, total_covariance_factor=0.0, covariance_floor=1e-6):
    """ivector-compute-lda from statistics, fp64: tot = sum over the utterances of v v^T (v the centred vectors), btw_means [K, d] the
    speakers' averages of v, counts [K].  -> (matrix [dim, d + 1] = [A | -A mu'], the eigenvalues l of the between-class covariance in the
    whitened space, descending, all d of them)."""
    tot = np.asarray(tot, dtype=np.float64)
    means = np.asarray(btw_means, dtype=np.float64)
    counts = np.asarray(counts, dtype=np.float64)
    d = tot.shape[0]
    if not 0 < dim <= d:
        raise ValueError("estimate_lda: dim must lie in 1 .. %d (got %d)" % (d, dim))
    n = counts.sum()
    btw = (means * counts[:, None]).T @ means
    total = tot / n
    within = (tot - btw) / n
    f = float(total_covariance_factor)
    s, u = np.linalg.eigh(f * total + (1.0 - f) * within)
    s = np.maximum(s, s.max() * covariance_floor)
    t = (u / np.sqrt(s)).T                                   # diag(s^-1/2) U^T
    l, v = _sym_eigh_desc(t @ (total - within) @ t.T)
    a = v[:, :dim].T @ t
    mu = counts @ means / n                                  # the mean of the already centred input: about 0
    return np.concatenate([a, -(a @ mu)[:, None]], axis=1), l


def estimate_plda(scatter, means, counts, num_em_iters=10):
    """ivector-compute-plda from statistics, fp64: scatter = sum over the utterances of y y^T (not centred), means [K, d] the speakers'
    averages of y, counts [K] (speakers with one utterance included).  The EM visits the speakers grouped by their count, so
    M_n = (B^-1 + n W^-1)^-1 is computed once per distinct n.  -> dict(mean, transform, psi, offset, within, between)."""
    means = np.asarray(means, dtype=np.float64)
    cnt = np.asarray(counts, dtype=np.int64)
    k, d = means.shape
    nf = cnt.astype(np.float64)
    s = np.asarray(scatter, dtype=np.float64) - (means * nf[:, None]).T @ means
    s = 0.5 * (s + s.T)
    mu = means.sum(axis=0) / k
    m_all = means - mu
    groups = [(int(n), np.nonzero(cnt == n)[0]) for n in np.unique(cnt)]
    w, b = np.eye(d), np.eye(d)
    for _ in range(int(num_em_iters)):
        w_inv, b_inv = np.linalg.inv(w), np.linalg.inv(b)
        wst, wc = s.copy(), float(nf.sum() - k)
        bst, bc = np.zeros((d, d)), 0.0
        for n, idx in groups:
            mn = np.linalg.inv(b_inv + n * w_inv)
            m = m_all[idx]
            ww = (n * (m @ w_inv.T)) @ mn.T                  # rows: M_n (n W^-1 m)
            r = m - ww
            bst += len(idx) * mn + ww.T @ ww
            wst += n * len(idx) * mn + n * (r.T @ r)
            bc += len(idx)
            wc += len(idx)
        w, b = wst / wc, bst / bc
        w, b = 0.5 * (w + w.T), 0.5 * (b + b.T)
    t1 = np.linalg.inv(np.linalg.cholesky(w))
    psi, u = _sym_eigh_desc(t1 @ b @ t1.T)
    psi = np.maximum(psi, 0.0)
    transform = u.T @ t1
    return dict(mean=mu, transform=transform, psi=psi, offset=-(transform @ mu), within=w, between=b)


def adapt_plda(plda, mean_y, scatter_y, n, within_covar_scale=0.3, between_covar_scale=0.7, mean_diff_scale=1.0):
    """ivector-adapt-plda from statistics, fp64 (INTEGRATION.md section 6b states the steps): plda = the model to adapt (mean, transform,
    psi), mean_y [d] = the average of the n adaptation vectors y (at ivector-normalize-length's scale, as Backend.train feeds its PLDA),
    scatter_y = sum y y^T (not centred).  The adaptation set's total covariance is whitened by the model's own; along each direction in which
    it exceeds 1, within_covar_scale / between_covar_scale of the excess go to the within- / between-class covariance.
    -> dict(mean, transform, psi, offset, within, between, eigenvalues = the s of the whitened covariance, descending)."""
    if within_covar_scale < 0 or between_covar_scale < 0 or mean_diff_scale < 0:
        raise ValueError("adapt_plda: the scales must not be negative (within %g, between %g, mean-diff %g)"
                         % (within_covar_scale, between_covar_scale, mean_diff_scale))
    mean, t, psi = (np.asarray(plda[k], dtype=np.float64) for k in ("mean", "transform", "psi"))
    m = np.asarray(mean_y, dtype=np.float64)
    d = m.shape[0]
    if mean.shape != (d,) or t.shape != (d, d) or psi.shape != (d,) or np.shape(scatter_y) != (d, d) or n <= 0:
        raise ValueError("adapt_plda: the model and the statistics must share one dimension, n must be positive")
    diff = m - mean
    v = np.asarray(scatter_y, dtype=np.float64) / float(n) - np.outer(m, m) + float(mean_diff_scale) * np.outer(diff, diff)
    mt = t / np.sqrt(1.0 + psi)[:, None]                       # the map under which the model's total covariance is the unit matrix
    s, p = _sym_eigh_desc(mt @ v @ mt.T)
    w2 = p.T @ (p / (1.0 + psi)[:, None])
    b2 = p.T @ (p * (psi / (1.0 + psi))[:, None])
    excess = np.maximum(s - 1.0, 0.0)
    w2[np.diag_indices(d)] += float(within_covar_scale) * excess
    b2[np.diag_indices(d)] += float(between_covar_scale) * excess
    k = np.linalg.inv(p.T @ mt)
    w, b = k @ w2 @ k.T, k @ b2 @ k.T
    w, b = 0.5 * (w + w.T), 0.5 * (b + b.T)
    t1 = np.linalg.inv(np.linalg.cholesky(w))
    psi_new, u = _sym_eigh_desc(t1 @ b @ t1.T)
    psi_new = np.maximum(psi_new, 0.0)
    transform = u.T @ t1
    return dict(mean=m, transform=transform, psi=psi_new, offset=-(transform @ m), within=w, between=b, eigenvalues=s)


def plda_coefficients(psi, distinct_n):
    """The tables of xv_backend_plda_trials for the utterance counts distinct_n, built in fp64 and rounded once: coef float32
    [len(distinct_n), 2, ldc] = (a = n psi / (n psi + 1), iv = 1 / v with v = 1 + psi / (n psi + 1)), g float32 [ldc] = 1 / (psi + 1),
    k0 float32 [len(distinct_n)] = -0.5 sum log v + 0.5 sum log(psi + 1); ldc = d rounded up to 4, the padding zero."""
    psi = np.asarray(psi, dtype=np.float64)
    d = psi.shape[0]
    ldc = pitch4(d)
    n = np.asarray(distinct_n, dtype=np.float64)[:, None]
    if n.size == 0 or n.min() < 1:
        raise ValueError("plda_coefficients: utterance counts must be positive")
    v = 1.0 + psi / (n * psi + 1.0)
    coef = np.zeros((n.shape[0], 2, ldc), np.float32)
    coef[:, 0, :d] = n * psi / (n * psi + 1.0)
    coef[:, 1, :d] = 1.0 / v
    g = np.zeros(ldc, np.float32)
    g[:d] = 1.0 / (psi + 1.0)
    k0 = (-0.5 * np.log(v).sum(axis=1) + 0.5 * np.log(psi + 1.0).sum()).astype(np.float32)
    return coef, g, k0


def plda_covariances(plda):
    """(W, B, mu) of a PLDA model (mean, transform T, psi), fp64: the within-class covariance W = T^-1 T^-T and the between-class covariance
    B = T^-1 diag(psi) T^-T, both symmetrised, and the mean - what xv_backend_pca_plda projects into a recording's subspace."""
    t_inv = np.linalg.inv(np.asarray(plda["transform"], dtype=np.float64))
    w, b = t_inv @ t_inv.T, (t_inv * np.asarray(plda["psi"], dtype=np.float64)[None, :]) @ t_inv.T
    return 0.5 * (w + w.T), 0.5 * (b + b.T), np.asarray(plda["mean"], dtype=np.float64)


PCA_NO_TARGET = 0.001      # a target energy this close to 1 means no PCA at all (ivector-plda-scoring-dense returns early)


def check_target_energy(target_energy, what):
    """None, or the target energy as a float in (0, 1]; anything else is refused in the name of `what`."""
    if target_energy is None:
        return None
    t = float(target_energy)
    if not 0.0 < t <= 1.0:
        raise ValueError("%s: target_energy must lie in (0, 1] (got %r)" % (what, target_energy))
    return t


def _device_rows(torch, matrix, device, d, what):
    """A [rows, >= d] float32 device matrix from a host matrix (uploaded) or a device tensor (taken as it is)."""
    if isinstance(matrix, torch.Tensor):
        if matrix.dim() != 2 or matrix.shape[0] == 0 or matrix.shape[1] < d:
            raise ValueError("%s: a non-empty [n, >= %d] matrix is expected" % (what, d))
        return matrix
    matrix = np.ascontiguousarray(matrix, dtype=np.float32)
    if matrix.ndim != 2 or matrix.shape[0] == 0 or matrix.shape[1] != d:
        raise ValueError("%s: a non-empty [n, %d] matrix is expected, got %s" % (what, d, matrix.shape))
    return torch.from_numpy(matrix).to(device)


class _Chain(object):
    """The device form of a Backend: centre -> LDA -> length normalisation (-> PLDA transform -> PLDA normalisation), in row batches."""

    def __init__(self, backend, device):
        self.torch, self.ops, self.device = device_ops(device)
        self.d, self.dim = backend.d, backend.dim
        up = lambda a: upload(a, np.float32, self.device)
        d4, k4 = pitch4(self.d), pitch4(self.dim)
        self.mean = up(backend.mean)
        self.lda_w = self.lda_b = self.plda_w = self.plda_b = self.psi = None
        if backend.lda is not None:
            w = np.zeros((k4, d4), np.float32)
            w[:self.dim, :self.d] = backend.lda[:, :self.d]
            b = np.zeros(k4, np.float32)
            b[:self.dim] = backend.lda[:, self.d]
            self.lda_w, self.lda_b = up(w), up(b)
        if backend.plda is not None:
            w = np.zeros((k4, k4), np.float64)
            w[:self.dim, :self.dim] = np.sqrt(float(self.dim)) * backend.plda["transform"]      # sqrt(dim) folded in before the one rounding
            b = np.zeros(k4, np.float64)
            b[:self.dim] = -(backend.plda["transform"] @ backend.plda["mean"])
            self.plda_w, self.plda_b, self.psi = up(w), up(b), up(backend.plda["psi"])

    def unit(self, x):
        """Centred, LDA-transformed (when the back end has one), unit-length rows on a zero-padded pitch."""
        ops = self.ops
        if self.lda_w is None:
            return ops.score_prepare(x, d=self.d, mean=self.mean)
        z = ops.backend_affine(ops.backend_center(x, d=self.d, mean=self.mean), self.lda_w, self.lda_b)
        return ops.score_prepare(z, d=self.dim, out=z)

    def plda(self, unit, n_utts=None):
        u = self.ops.backend_affine(unit, self.plda_w, self.plda_b)
        return self.ops.backend_plda_normalize(u, self.dim, self.psi, n_utts=n_utts, out=u)

    def run(self, x, plda, n_utts=None):
        parts = []
        for r0, r1 in steps(x.shape[0], PREPARE_ROWS):
            y = self.unit(x[r0:r1])
            parts.append(self.plda(y, None if n_utts is None else n_utts[r0:r1]) if plda else y)
        return cat(parts)


class Backend(object):
    """A trained back end: the global mean (float32 [d]), the LDA matrix (float32 [dim, d + 1], None without LDA) and the PLDA model
    (float64 mean [dim], transform [dim, dim], psi [dim]; None for an LDA-only directory).  save / load use the recipe's file names:
    mean.vec, transform.mat, plda."""

    def __init__(self, mean, lda=None, plda=None):
        self.mean = np.ascontiguousarray(mean, dtype=np.float32)
        self.lda = None if lda is None else np.ascontiguousarray(lda, dtype=np.float32)
        self.plda = None if plda is None else {k: np.ascontiguousarray(plda[k], dtype=np.float64) for k in ("mean", "transform", "psi")}
        self.d = self.mean.shape[0]
        if self.lda is not None and (self.lda.ndim != 2 or self.lda.shape[1] != self.d + 1):
            raise ValueError("Backend: the LDA matrix must be [dim, %d] (d + 1 columns), got %s" % (self.d + 1, self.lda.shape))
        self.dim = self.d if self.lda is None else self.lda.shape[0]
        if self.plda is not None and self.plda["mean"].shape[0] != self.dim:
            raise ValueError("Backend: the PLDA model works on %d dimensions, the vectors in front of it have %d" % (self.plda["mean"].shape[0], self.dim))

    def save(self, directory):
        kaldi_io = _kaldi_io()
        os.makedirs(directory, exist_ok=True)
        kaldi_io.write_vec_flt(os.path.join(directory, "mean.vec"), self.mean)
        if self.lda is not None:
            kaldi_io.write_mat(os.path.join(directory, "transform.mat"), self.lda)
        if self.plda is not None:
            kaldi_io.write_plda(os.path.join(directory, "plda"), self.plda["mean"], self.plda["transform"], self.plda["psi"])

    @classmethod
    def load(cls, directory):
        kaldi_io = _kaldi_io()
        path = lambda name: os.path.join(directory, name)
        if not os.path.isfile(path("mean.vec")):
            raise ValueError("%s: no mean.vec: not a back-end directory (nnet/lib/train_backend.py writes one)" % directory)
        mean = np.asarray(kaldi_io.read_vec_flt(path("mean.vec")), dtype=np.float32)
        lda = np.asarray(kaldi_io.read_mat(path("transform.mat")), dtype=np.float32) if os.path.isfile(path("transform.mat")) else None
        plda = None
        if os.path.isfile(path("plda")):
            plda = dict(zip(("mean", "transform", "psi"), kaldi_io.read_plda(path("plda"))))
        return cls(mean, lda, plda)

    @classmethod
    def train(cls, matrix, keys, spk2utt, lda_dim=200, device="cuda:0", num_em_iters=10, log=None):
        """Train on the table (keys, matrix float32 [n, d]) grouped by spk2utt (read_spk2utt's list); lda_dim None / 0: no LDA.  The
        statistics come from the GPU (xv_backend_group_means, xv_backend_scatter, the transform chain), the estimators run here in fp64."""
        torch, ops, _ = device_ops(device)
        log = log or _LOG
        matrix = np.ascontiguousarray(matrix, dtype=np.float32)
        groups = GroupIndex(keys, spk2utt, log)
        if len(groups) == 0:
            raise ValueError("Backend.train: no speaker of the spk2utt has a vector")
        d = matrix.shape[1]
        mean = center_mean(matrix).astype(np.float32)
        x = torch.from_numpy(matrix).to(device)
        # (rows no speaker lists enter the global mean as in the recipe - ivector-mean reads the whole table - but no scatter)
        listed = np.unique(groups.rows)
        if listed.size != matrix.shape[0]:
            log.info("[INFO] %d of %d vectors belong to no speaker of the spk2utt: they enter the mean only." % (matrix.shape[0] - listed.size, matrix.shape[0]))
            x_stats = x[torch.from_numpy(listed.astype(np.int64)).to(device)]
            remap = np.full(matrix.shape[0], -1, np.int64)
            remap[listed] = np.arange(listed.size)
            rows = remap[groups.rows].astype(np.int32)
        else:
            x_stats, rows = x, groups.rows
        counts = groups.counts
        log.info("[INFO] Back end: N = %d vectors of K = %d speakers, d = %d." % (int(counts.sum()), len(groups), d))
        lda = None
        mean_d = torch.from_numpy(mean).to(device)
        if lda_dim:
            if not 0 < lda_dim <= d:
                raise ValueError("Backend.train: lda_dim must lie in 1 .. %d (got %d)" % (d, lda_dim))
            v = ops.backend_center(x_stats, mean=mean_d)
            tot = ops.backend_scatter(v, d=d).cpu().numpy()
            m64 = ops.backend_group_means(v, d, groups.offsets, rows, want32=False)[0].cpu().numpy()
            lda, l = estimate_lda(tot, m64, counts, int(lda_dim))
            log.info("[INFO] LDA: kept eigenvalues %.6g .. %.6g (the next one: %s)." % (l[0], l[lda_dim - 1], "%.6g" % l[lda_dim] if lda_dim < d else "none"))
        self = cls(mean, lda, None)
        chain = _Chain(self, device)
        y = cat([chain.unit(x_stats[r0:r1]) for r0, r1 in steps(x_stats.shape[0], PREPARE_ROWS)])
        # y is at unit length; the model is trained at ivector-normalize-length's scale sqrt(dim): both statistics are scaled here, in fp64
        scatter = ops.backend_scatter(y, d=self.dim).cpu().numpy() * float(self.dim)
        m64 = ops.backend_group_means(y, self.dim, groups.offsets, rows, want32=False)[0].cpu().numpy() * np.sqrt(float(self.dim))
        plda = estimate_plda(scatter, m64, counts, num_em_iters)
        log.info("[INFO] PLDA: psi min %.6g, max %.6g (%d EM iterations)." % (plda["psi"].min(), plda["psi"].max(), num_em_iters))
        return cls(mean, lda, plda)

    def recentred(self, matrix):
        """This back end on the mean of another table (the fp64-accumulated mean.vec of `matrix`), nothing adapted: the recipe's
        out-of-domain PLDA on the in-domain mean (egs/sre/v1/run.sh:477-483)."""
        matrix = np.ascontiguousarray(matrix, dtype=np.float32)
        if matrix.ndim != 2 or matrix.shape[0] == 0 or matrix.shape[1] != self.d:
            raise ValueError("Backend.recentred: dimension mismatch: a non-empty [n, %d] matrix is expected, got %s" % (self.d, matrix.shape))
        return Backend(center_mean(matrix).astype(np.float32), self.lda, self.plda)

    def adapt(self, matrix, device="cuda:0", within_covar_scale=0.3, between_covar_scale=0.7, mean_diff_scale=1.0, log=None):
        """ivector-adapt-plda on the unlabelled table `matrix` [n, d] (egs/sre/v1/run.sh:451-492): the new mean.vec is the table's mean, the
        LDA is kept, and the PLDA model is adapted to the table's vectors taken through the chain centred on the NEW mean.  Their
        statistics come from the GPU in PREPARE_ROWS batches (the transform chain, xv_backend_scatter, and xv_backend_group_means with a
        single group for the row sum in double); adapt_plda runs here in fp64.  -> Backend(new mean, lda, adapted plda)."""
        if self.plda is None:
            raise ValueError("Backend.adapt: the back end holds no PLDA model (no `plda` file in its directory)")
        torch, ops, _ = device_ops(device)
        log = log or _LOG
        base = self.recentred(matrix)
        matrix = np.ascontiguousarray(matrix, dtype=np.float32)
        chain = _Chain(Backend(base.mean, self.lda, None), device)
        n, dim = matrix.shape[0], self.dim
        scatter, total = np.zeros((dim, dim)), np.zeros(dim)
        for r0, r1 in steps(n, PREPARE_ROWS):
            y = chain.unit(torch.from_numpy(matrix[r0:r1]).to(device))
            scatter += ops.backend_scatter(y, d=dim).cpu().numpy()
            one = ops.backend_group_means(y, dim, np.array([0, r1 - r0], np.int64), np.arange(r1 - r0, dtype=np.int32), want32=False)[0]
            total += one.cpu().numpy()[0] * float(r1 - r0)
        # y is at unit length; the model works at ivector-normalize-length's scale sqrt(dim): both statistics are scaled here, in fp64
        plda = adapt_plda(self.plda, total / n * np.sqrt(float(dim)), scatter * float(dim), n, within_covar_scale, between_covar_scale,
                          mean_diff_scale)
        s = plda["eigenvalues"]
        log.info("[INFO] PLDA adaptation: N = %d vectors, %d of %d eigenvalues above 1 (largest %.6g, smallest %.6g); psi min %.6g, max %.6g."
                 % (n, int((s > 1.0).sum()), dim, s[0], s[-1], plda["psi"].min(), plda["psi"].max()))
        return Backend(base.mean, self.lda, plda)


class BackendScorer(object):
    """Trial scores behind a trained back end, the tables kept on the GPU as CosineScorer keeps them.

        scorer = BackendScorer(backend, "plda", "cuda:0")            # or "lda_cos": cosine behind centring and the LDA
        names, avg, counts = scorer.enrol_average(matrix, keys, spk2utt)   # optional: models = averages of raw vectors (ivector-mean ark:spk2utt)
        enrol = scorer.prepare(avg, n_utts=counts)                   # host [n, d] matrix or device tensor -> prepared device matrix
        test = scorer.prepare(test_matrix)
        scorer.cohort(cohort_matrix, top_k=300)                      # optional, "plda" mode: AS-norm of the log-likelihood ratios; cohort(None) drops it
        scores = scorer.score(enrol, test, ei, ti, enrol_n=counts)   # NumPy float32 [m]

    n_utts / enrol_n (None: 1 per row) enter the "plda" mode only: the normalisation of an enrolment vector and its log-likelihood ratio.
    With a cohort every score s becomes 0.5 * ((s - mu_e) / sigma_e + (s - mu_t) / sigma_t): mu / sigma the mean and deviation of the top_k
    largest ratios of the enrolment model (with its utterance count) / of the test vector (as a one-utterance model) against the cohort
    vectors (xv_backend_plda_cohort_stats).  score() cuts the trials, and the rows whose cohort statistics it needs, into batches such that
    no call asks for more than workspace_bytes of scratch."""

    MODES = ("lda_cos", "plda")
    _cohort, top_k = None, 0      # no cohort until cohort() sets one
    _dense_tables = None          # the one-utterance coefficient tables on the device, built by the first dense()
    _pca_model = None             # (W, B, mean) of the PLDA model in float64 on the device, built by the first prepare_pca()

    def __init__(self, backend, mode="plda", device="cuda:0", workspace_bytes=DEFAULT_WORKSPACE_BYTES):
        if mode not in self.MODES:
            raise ValueError("BackendScorer: mode must be one of %s (got %r)" % (", ".join(self.MODES), mode))
        if mode == "plda" and backend.plda is None:
            raise ValueError("BackendScorer: the back end holds no PLDA model (no `plda` file in its directory)")
        self.mode, self.backend = mode, backend
        self.chain = _Chain(backend, device)
        self.torch, self.ops, self.device = self.chain.torch, self.chain.ops, self.chain.device
        self.workspace_bytes = int(workspace_bytes)
        self.d, self.dim = backend.d, backend.dim

    def cohort(self, matrix, top_k=0):
        """The cohort of AS-norm: prepared with one utterance per row and kept on the device.  matrix None: no cohort any more."""
        if matrix is None:
            self._cohort, self.top_k = None, 0
            return
        if self.mode != "plda":
            raise ValueError("BackendScorer.cohort: AS-norm of PLDA scores needs the plda mode (lda_cos: CosineScorer on the prepared tables)")
        if int(top_k) <= 0:
            raise ValueError("BackendScorer.cohort: top_k must be positive (got %d)" % top_k)
        self._cohort, self.top_k = self.prepare(matrix), int(top_k)

    def _stats(self, x, nidx, tables):
        """Cohort statistics [n, 2] of the prepared rows x (table entries nidx; None: entry 0), in row batches that fit the workspace."""
        n_cohort, nq = self._cohort.shape[0], tables[0].shape[0]
        need = lambda rows: self.ops.backend_plda_cohort_workspace_bytes(rows, n_cohort, self.dim, nq)
        tile = need(256) - need(128)                            # what 128 more rows cost; the rest of need(128) are the column terms
        if need(128) > self.workspace_bytes:
            raise ValueError("BackendScorer: a workspace of %d bytes does not hold one 128-row tile of %d cohort scores (%d bytes)"
                             % (self.workspace_bytes, n_cohort, need(128)))
        step = (self.workspace_bytes - (need(128) - tile)) // tile * 128
        return cat([self.ops.backend_plda_cohort_stats(x[r0:r1], self._cohort, self.dim, None if nidx is None else nidx[r0:r1], *tables,
                                                       top_k=self.top_k, ws_bytes=need(r1 - r0))
                    for r0, r1 in steps(x.shape[0], step)])

    def enrol_average(self, matrix, keys, spk2utt, log=None):
        """(names, device float32 [models, d rounded up to 4], counts int64): per speaker of spk2utt the plain average of its raw vectors,
        accumulated in fp64 in list order and rounded once (xv_backend_group_means), and how many there were."""
        groups = GroupIndex(keys, spk2utt, log)
        if len(groups) == 0:
            raise ValueError("BackendScorer.enrol_average: no speaker of the spk2utt has a vector")
        x = _device_rows(self.torch, matrix, self.device, self.d, "BackendScorer.enrol_average")
        return groups.names, self.ops.backend_group_means(x, self.d, groups.offsets, groups.rows)[1], groups.counts

    def prepare(self, matrix, n_utts=None):
        x = _device_rows(self.torch, matrix, self.device, self.d, "BackendScorer.prepare")
        if n_utts is not None and len(n_utts) != x.shape[0]:
            raise ValueError("BackendScorer.prepare: n_utts must hold one count per row (%d, got %d)" % (x.shape[0], len(n_utts)))
        return self.chain.run(x, self.mode == "plda", None if n_utts is None else np.asarray(n_utts))

    def plda_space(self, matrix):
        """The rows of `matrix` (host [n, d] or device tensor, raw vectors as prepare takes them) in the space of the PLDA model, where the
        within-class covariance is I and the between-class covariance diag(psi): centred, LDA-transformed, length-normalised and taken
        through the PLDA transform, WITHOUT backend_plda_normalize - what ops.vbx models.  -> (device float32 [n, dim rounded up to 4],
        psi device float32 [dim])."""
        if self.backend.plda is None or self.mode != "plda":
            raise ValueError("BackendScorer.plda_space: needs a PLDA model and the plda mode (this scorer: mode %s, %s)"
                             % (self.mode, "no PLDA model" if self.backend.plda is None else "with a PLDA model"))
        x = _device_rows(self.torch, matrix, self.device, self.d, "BackendScorer.plda_space")
        chain = self.chain
        rows = cat([self.ops.backend_affine(chain.unit(x[r0:r1]), chain.plda_w, chain.plda_b) for r0, r1 in steps(x.shape[0], PREPARE_ROWS)])
        return rows, chain.psi

    def prepare_pca(self, matrices, target_energy):
        """The recordings of one batch behind ivector-plda-scoring-dense's per-recording PCA (ops.backend_pca_plda: one call for the batch).
        matrices: the raw vectors of each recording (host [n, d] or device tensors, as prepare takes them); target_energy in (0, 1].
        -> per recording (prepared rows, model): model = (p, coef, g, k0), the kept dimension and the recording's own one-utterance tables
        for dense(prepared, model=model), the rows taken through the recording's map and normalised with its psi; model None where the
        recording is scored with the global model (prepare's rows): a single row, a zero covariance, or a target within 0.001 of 1 - then
        the op is not called at all."""
        if self.mode != "plda":
            raise ValueError("BackendScorer.prepare_pca: the per-recording PCA needs the plda mode (this scorer: mode %s)" % self.mode)
        target = check_target_energy(target_energy, "BackendScorer.prepare_pca")
        if target is None:
            raise ValueError("BackendScorer.prepare_pca: target_energy must lie in (0, 1] (got None)")
        torch, ops, chain = self.torch, self.ops, self.chain
        units = [chain.unit(_device_rows(torch, m, self.device, self.d, "BackendScorer.prepare_pca")) for m in matrices]
        if not units or target > 1.0 - PCA_NO_TARGET:
            return [(chain.plda(u), None) for u in units]
        if self._pca_model is None:
            self._pca_model = tuple(upload(a, np.float64, self.device) for a in plda_covariances(self.backend.plda))
        x, offsets, n, ld = pack_rows(units)
        got = ops.backend_pca_plda(x, offsets, n, self.dim, *self._pca_model, target=target, ld=ld)
        kept = got["p"].cpu().numpy()
        out = []
        for j, u in enumerate(units):
            p = int(kept[j])
            if p < 0:
                raise RuntimeError("BackendScorer.prepare_pca: xv_backend_pca_plda gave up on recording %d of the batch (p = %d: %s)"
                                   % (j, p, {-1: "its rows lie outside the call's buffer", -2: "the eigensolver reached its sweep cap",
                                             -3: "the projected within-class covariance is not positive definite"}.get(p, "unknown")))
            if p == 0:
                out.append((chain.plda(u), None))
                continue
            p4 = pitch4(p)
            y = ops.backend_affine(u, got["a"][j, :p4], got["offset"][j, :p4])
            y = ops.backend_plda_normalize(y, p, got["psi"][j, :p], out=y)
            out.append((y, (p, got["coef"][j:j + 1], got["g"][j], got["k0"][j:j + 1])))
        return out

    def dense(self, prepared, out=None, model=None):
        """The score of every pair of the prepared rows (one utterance each), a device float32 [n, n] matrix: the cosine in the lda_cos mode
        (ops.score_dense), the log-likelihood ratio in the plda mode (ops.backend_plda_dense); no cohort enters.  out: a [n, n] view of any
        pitch to write - misc/diarization.py hands views into one packed buffer; default a new matrix.  model: a recording's own
        (p, coef, g, k0) from prepare_pca, with that call's rows; None: the global model."""
        if model is not None:
            if self.mode != "plda":
                raise ValueError("BackendScorer.dense: a per-recording model needs the plda mode (this scorer: mode %s)" % self.mode)
            return self.ops.backend_plda_dense(prepared, model[0], *model[1:], out=out)
        if self.mode == "lda_cos":
            return self.ops.score_dense(prepared, self.dim, out=out)
        if self._dense_tables is None:
            self._dense_tables = tuple(upload(a, np.float32, self.device) for a in plda_coefficients(self.backend.plda["psi"], [1]))
        return self.ops.backend_plda_dense(prepared, self.dim, *self._dense_tables, out=out)

    def score(self, enrol, test, ei, ti, enrol_n=None):
        ei, ti = np.asarray(ei), np.asarray(ti)
        step = max(self.workspace_bytes // 12, 1)      # two int32 indices and one score per trial
        if self.mode == "lda_cos":
            run = lambda a, b: self.ops.score_trials(enrol, test, self.dim, a, b)
        else:
            n = np.ones(enrol.shape[0], np.int64) if enrol_n is None else np.asarray(enrol_n, dtype=np.int64)
            if n.shape != (enrol.shape[0],):
                raise ValueError("BackendScorer.score: enrol_n must hold one count per enrolment row")
            if self._cohort is not None:
                distinct = np.unique(np.concatenate([[1], n]))      # the table always holds n = 1, as entry 0: the test side of AS-norm
                nidx = np.searchsorted(distinct, n)
            else:
                distinct, nidx = np.unique(n, return_inverse=True)
            coef, g, k0 = (upload(a, np.float32, self.device) for a in plda_coefficients(self.backend.plda["psi"], distinct))
            run = lambda a, b: self.ops.backend_plda_trials(enrol, test, self.dim, a, b, nidx, coef, g, k0)
            if self._cohort is not None:
                e_stats = self._stats(enrol, nidx, (coef, g, k0))
                t_stats = e_stats if test is enrol and not nidx.any() else self._stats(test, None, (coef, g, k0))

                def run(a, b, raw=run):      # the raw ratios of a batch, normalised in place
                    s = raw(a, b)
                    return self.ops.score_normalize(s, a, b, e_stats, t_stats, out=s)
        return cat([run(ei[j0:j1], ti[j0:j1]).cpu().numpy() for j0, j1 in steps(ei.shape[0], step)])
