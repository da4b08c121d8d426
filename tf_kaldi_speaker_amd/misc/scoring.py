"""Cosine trial scoring with adaptive symmetric score normalisation (AS-norm), the stage behind extraction (nnet/lib/score.py).

Host side: Kaldi trial lists, float-vector archives by key, EER and the normalised minimum detection cost.  Device side: CosineScorer,
which keeps prepared (centred, unit-length) embedding matrices on the GPU and runs the three kernels of csrc/xv_score.hip through ops.py.
LDA / PLDA and multi-utterance enrolment (spk2utt averaging): misc/backend.py.  Not here: DET plots.
"""
import numpy as np

try:
    from .._host import DEFAULT_WORKSPACE_BYTES, cat, device_ops, steps, upload
except (ImportError, ValueError):
    from _host import DEFAULT_WORKSPACE_BYTES, cat, device_ops, steps, upload

# (p_target, c_miss, c_fa) of the two detection costs in the reference's result tables: NIST SRE 2008 and 2010
MIN_DCF_PRESETS = {"minDCF08": (0.01, 10.0, 1.0), "minDCF10": (0.001, 1.0, 1.0)}


def read_trials(path):
    """Kaldi trial lines `enrol test [target|nontarget]` -> list of (enrol, test, label), label True / False / None (no third column).
    Blank lines are skipped; any other label, or a line of another width, is refused with its line number."""
    trials = []
    with open(path, "r") as f:
        for no, line in enumerate(f, 1):
            cols = line.split()
            if not cols:
                continue
            if len(cols) not in (2, 3):
                raise ValueError("%s:%d: a trial is `enrol test [target|nontarget]`, got %d columns" % (path, no, len(cols)))
            label = None
            if len(cols) == 3:
                if cols[2] not in ("target", "nontarget"):
                    raise ValueError("%s:%d: bad trial label %r (expected target or nontarget)" % (path, no, cols[2]))
                label = cols[2] == "target"
            trials.append((cols[0], cols[1], label))
    return trials


def read_vectors(rspecifier):
    """(keys, matrix float32 [n, d]) of a float-vector table written by write_vec_flt: `ark:FILE` (or a bare archive name) or `scp:FILE`.
    Vectors of different lengths inside one table are refused by name."""
    try:
        from ..dataset import kaldi_io
    except (ImportError, ValueError):
        from dataset import kaldi_io
    reader = kaldi_io.read_vec_flt_scp if rspecifier.startswith("scp:") else kaldi_io.read_vec_flt_ark
    keys, rows = [], []
    for key, vec in reader(rspecifier):
        if rows and vec.shape[0] != rows[0].shape[0]:
            raise ValueError("%s: vector %s has %d dimensions, the ones before it %d" % (rspecifier, key, vec.shape[0], rows[0].shape[0]))
        keys.append(key)
        rows.append(np.asarray(vec, dtype=np.float32))
    if not rows:
        raise ValueError("%s: no vectors" % rspecifier)
    return keys, np.stack(rows)


def center_mean(matrix):
    """The mean a table is centred on (ivector-mean), accumulated in fp64."""
    return np.asarray(matrix, dtype=np.float64).mean(axis=0)


def index_trials(trials, enrol_keys, test_keys):
    """Row indices of the trials whose two keys exist, in trial order: (kept trials, ei int32, ti int32, skipped trials)."""
    e_at = {k: i for i, k in enumerate(enrol_keys)}
    t_at = e_at if test_keys is enrol_keys else {k: i for i, k in enumerate(test_keys)}
    kept, ei, ti, skipped = [], [], [], []
    for trial in trials:
        a, b = e_at.get(trial[0]), t_at.get(trial[1])
        if a is None or b is None:
            skipped.append(trial)
            continue
        kept.append(trial)
        ei.append(a)
        ti.append(b)
    return kept, np.asarray(ei, dtype=np.int32), np.asarray(ti, dtype=np.int32), skipped


def compute_eer(scores, targets):
    """Equal error rate of scores against 0 / 1 targets: the root of 1 - x - tpr(x) on the ROC curve (reference utils.py:309-312)."""
    from scipy.interpolate import interp1d
    from scipy.optimize import brentq
    from sklearn import metrics
    fpr, tpr, _ = metrics.roc_curve(targets, scores, pos_label=1)
    return float(brentq(lambda x: 1.0 - x - interp1d(fpr, tpr)(x), 0.0, 1.0))


def compute_min_dcf(scores, targets, p_target, c_miss, c_fa):
    """Normalised minimum detection cost: min over thresholds (a trial is accepted when its score >= threshold; every distinct score and
    "accept nothing") of c_miss * p_target * P_miss + c_fa * (1 - p_target) * P_fa, divided by min(c_miss * p_target, c_fa * (1 - p_target))."""
    scores = np.asarray(scores, dtype=np.float64)
    targets = np.asarray(targets).astype(bool)
    n_tar, n_non = int(targets.sum()), int((~targets).sum())
    if n_tar == 0 or n_non == 0:
        raise ValueError("compute_min_dcf: the trials need at least one target and one nontarget")
    order = np.argsort(-scores, kind="stable")
    s, t = scores[order], targets[order]
    last = np.r_[s[1:] != s[:-1], True]                      # the last trial of each run of equal scores: a threshold sits below the run
    tp = np.r_[0, np.cumsum(t)[last]].astype(np.float64)      # (leading 0: the threshold above every score)
    fp = np.r_[0, np.cumsum(~t)[last]].astype(np.float64)
    cost = c_miss * p_target * (1.0 - tp / n_tar) + c_fa * (1.0 - p_target) * (fp / n_non)
    return float(cost.min() / min(c_miss * p_target, c_fa * (1.0 - p_target)))


class CosineScorer(object):
    """Cosine scores of trials between two embedding tables, AS-normalised when a cohort is set.

        scorer = CosineScorer("cuda:0", center=mean)       # mean: [d], subtracted from every vector (cohort included); None: nothing
        enrol = scorer.prepare(matrix)                       # [n, d] host matrix -> prepared device matrix
        scorer.cohort(cohort_matrix, top_k=300)              # optional
        scores = scorer.score(enrol, test, ei, ti)           # NumPy float32 [m], trial j = enrol row ei[j] against test row ti[j]

    score() cuts the trials and the rows whose cohort statistics it needs into batches such that no single call asks for more than
    workspace_bytes of scratch (index arrays and scores of a trial batch; the score slab of a row batch)."""

    def __init__(self, device="cuda:0", center=None, workspace_bytes=DEFAULT_WORKSPACE_BYTES):
        self.torch, self.ops, self.device = device_ops(device)
        self.workspace_bytes = int(workspace_bytes)
        self.d = None
        self.center = None if center is None else upload(center, np.float32, self.device)
        self._cohort, self.top_k = None, 0

    def prepare(self, matrix):
        matrix = np.ascontiguousarray(matrix, dtype=np.float32)
        if matrix.ndim != 2 or matrix.shape[0] == 0 or matrix.shape[1] == 0:
            raise ValueError("CosineScorer.prepare: a non-empty [n, d] matrix is expected")
        if self.d is None:
            self.d = matrix.shape[1]
        if matrix.shape[1] != self.d or (self.center is not None and self.center.numel() != self.d):
            raise ValueError("CosineScorer.prepare: dimension mismatch: this matrix has d = %d, the scorer works on d = %d%s"
                             % (matrix.shape[1], self.d, "" if self.center is None else " (centre: %d)" % self.center.numel()))
        return self.ops.score_prepare(self.torch.from_numpy(matrix).to(self.device), mean=self.center)

    def cohort(self, matrix, top_k):
        if int(top_k) <= 0:
            raise ValueError("CosineScorer.cohort: top_k must be positive (got %d)" % top_k)
        self._cohort, self.top_k = self.prepare(matrix), int(top_k)

    def _stats(self, x):
        """Cohort statistics [n, 2] of the prepared rows x, in row batches whose score slab fits the workspace."""
        n_cohort = self._cohort.shape[0]
        tile = self.ops.score_cohort_workspace_bytes(128, n_cohort, self.d)
        if tile > self.workspace_bytes:
            raise ValueError("CosineScorer: a workspace of %d bytes does not hold one 128-row tile of %d cohort scores (%d bytes)"
                             % (self.workspace_bytes, n_cohort, tile))
        step = self.workspace_bytes // tile * 128
        return cat([self.ops.score_cohort_stats(x[r0:r1], self._cohort, self.d, self.top_k,
                                                      ws_bytes=self.ops.score_cohort_workspace_bytes(r1 - r0, n_cohort, self.d))
                          for r0, r1 in steps(x.shape[0], step)])

    def dense(self, prepared, out=None):
        """The cosine of every pair of the prepared rows, a device float32 [n, n] matrix (ops.score_dense; no cohort enters).  out: a
        [n, n] view of any pitch to write - misc/diarization.py hands views into one packed buffer; default a new matrix."""
        return self.ops.score_dense(prepared, self.d, out=out)

    def score(self, enrol, test, ei, ti):
        ei, ti = np.asarray(ei), np.asarray(ti)
        e_stats = t_stats = None
        if self._cohort is not None:
            e_stats = self._stats(enrol)
            t_stats = e_stats if test is enrol else self._stats(test)
        step = max(self.workspace_bytes // 12, 1)      # two int32 indices and one score per trial
        return cat([self.ops.score_trials(enrol, test, self.d, ei[j0:j1], ti[j0:j1], e_stats, t_stats).cpu().numpy()
                          for j0, j1 in steps(ei.shape[0], step)])
