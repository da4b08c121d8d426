"""Speaker diarization behind the x-vector network and the scoring back ends (nnet/lib/diarize.py): what Kaldi's callhome_diarization/v2
recipe does around its x-vectors - sliding sub-segments, all-pairs scores per recording, agglomerative clustering, RTTM - restated;
nothing is compared with a Kaldi run.

Host side, NumPy only: speech segments from VAD decisions or a `segments` file, the window planner, the turns of an RTTM from clustered
windows, RTTM files and a plain diarization error rate.  Device side: Diarizer, which takes the windows' embeddings of many recordings
through a scorer's prepare -> dense into one packed buffer and clusters them in one ops.ahc_cluster call per batch; with VbxOptions the
clusterer's labels start the VB-HMM clustering of the windows (VBx, ops.vbx: DESIGN.md section 6j) over the same batch; with target_energy
the PLDA scores of a recording come from its own model behind the per-recording PCA of ivector-plda-scoring-dense
(ops.backend_pca_plda: DESIGN.md section 6k), one op call per batch; a recording of more than first_pass_max_points windows is clustered in
two passes (ops.ahc_cluster_two_pass: DESIGN.md section 6l), up to 32768 windows.
Not here: threshold calibration, overlap detection, collars / md-eval, VBx or the per-recording PCA on recordings of
more than 2048 windows.
"""
import logging

import numpy as np

_LOG = logging.getLogger("tf_kaldi_speaker_amd")
DER_FRAME = 0.01      # seconds per frame of der()
FIRST_PASS_CAP = 2048      # the most windows a subset of the first pass may hold: the clusterer's cap (ops.AHC_MAX_N)


def speech_segments(vad, min_frames=1):
    """The maximal runs of voiced frames (vad[i] != 0) of at least min_frames frames -> list of (start, end), end exclusive."""
    v = np.concatenate([[False], np.asarray(vad) != 0, [False]])
    edges = np.flatnonzero(v[1:] != v[:-1])
    return [(int(s), int(e)) for s, e in zip(edges[0::2], edges[1::2]) if e - s >= min_frames]


def read_segments(path):
    """Kaldi `segments` lines `utterance recording start end` (seconds) -> list of (utterance, recording, start, end) in file order.  Blank
    lines are skipped; a line of another width, or an end that is not behind its start, is refused with its line number."""
    out = []
    with open(path, "r") as f:
        for no, line in enumerate(f, 1):
            cols = line.split()
            if not cols:
                continue
            if len(cols) not in (4, 5):      # (a fifth column is the channel: ignored)
                raise ValueError("%s:%d: a segment is `utterance recording start end`, got %d columns" % (path, no, len(cols)))
            start, end = float(cols[2]), float(cols[3])
            if not 0.0 <= start < end:
                raise ValueError("%s:%d: segment %s runs from %g to %g" % (path, no, cols[0], start, end))
            out.append((cols[0], cols[1], start, end))
    return out


def subsegments(start, end, window, period, min_segment, log=None):
    """The sliding windows of the segment [start, end), all in frames: window k starts at t_k = start + k * period and is
    [t_k, min(t_k + window, end)); the first window with t_k + window >= end is the last.  A window shorter than min_segment is kept only
    if it is the first; a segment shorter than min_segment gives none (a log line says so).  -> list of (start, end)."""
    start, end, window, period, min_segment = int(start), int(end), int(window), int(period), int(min_segment)
    if window <= 0 or period <= 0:
        raise ValueError("subsegments: window and period must be positive (got %d, %d)" % (window, period))
    if end - start < min_segment or end <= start:
        (log or _LOG).info("[INFO] Segment %d .. %d: %d frames, fewer than %d, dropped." % (start, end, end - start, min_segment))
        return []
    out, t, k = [], start, 0
    while True:
        stop = min(t + window, end)
        if stop - t >= min_segment or k == 0:
            out.append((t, stop))
        if t + window >= end:
            return out
        t, k = t + period, k + 1


def rttm_turns(subsegs, labels):
    """Speaker turns from clustered windows: subsegs [(start, end)] (any unit), labels one per window.  The windows are sorted by start;
    where two consecutive windows overlap, the first ends and the second starts at the midpoint of the overlap; then abutting windows of
    one label are merged.  -> list of (start, end, label)."""
    if len(subsegs) != len(labels):
        raise ValueError("rttm_turns: %d windows, %d labels" % (len(subsegs), len(labels)))
    order = sorted(range(len(subsegs)), key=lambda i: (subsegs[i][0], subsegs[i][1]))
    cut = [[float(subsegs[i][0]), float(subsegs[i][1]), int(labels[i])] for i in order]
    for a, b in zip(cut[:-1], cut[1:]):
        if a[1] > b[0]:
            a[1] = b[0] = 0.5 * (a[1] + b[0])
    turns = []
    for s, e, l in cut:
        if turns and turns[-1][2] == l and turns[-1][1] == s:
            turns[-1][1] = e
        else:
            turns.append([s, e, l])
    return [(s, e, l) for s, e, l in turns]


def write_rttm(path, turns_by_recording):
    """`SPEAKER <recording> 0 <start> <duration> <NA> <NA> <label + 1> <NA> <NA>` per turn; turns_by_recording: {recording: [(start, end,
    label)]} in seconds, written in the mapping's order."""
    with open(path, "w") as f:
        for reco, turns in turns_by_recording.items():
            for s, e, l in turns:
                f.write("SPEAKER %s 0 %.3f %.3f <NA> <NA> %d <NA> <NA>\n" % (reco, s, e - s, int(l) + 1))


def read_rttm(path):
    """{recording: [(start, end, speaker name)]} of the SPEAKER lines of an RTTM file, in file order; other line types are skipped, a
    SPEAKER line of fewer than 8 columns is refused with its line number."""
    out = {}
    with open(path, "r") as f:
        for no, line in enumerate(f, 1):
            cols = line.split()
            if not cols or cols[0] != "SPEAKER":
                continue
            if len(cols) < 8:
                raise ValueError("%s:%d: a SPEAKER line has at least 8 columns, got %d" % (path, no, len(cols)))
            start, dur = float(cols[3]), float(cols[4])
            out.setdefault(cols[1], []).append((start, start + dur, cols[7]))
    return out


def _frame_labels(turns, frames, names):
    lab = np.full(frames, -1, np.int64)
    for s, e, l in sorted(turns, key=lambda t: (t[0], t[1])):
        a, b = int(round(s / DER_FRAME)), int(round(e / DER_FRAME))
        span = lab[a:b]
        span[span < 0] = names.setdefault(l, len(names))      # overlapped speech: the first speaker only
    return lab


def der(ref, hyp):
    """Diarization error of the turns hyp against ref ([(start, end, speaker)] in seconds, one recording) on 10 ms frames, no collar;
    where turns of one side overlap, the frame goes to the turn that starts first.  The speakers are mapped one to one such that the
    matched time is largest (scipy.optimize.linear_sum_assignment).  -> (miss, false alarm, confusion, DER), fractions of the reference's
    speech time."""
    from scipy.optimize import linear_sum_assignment
    frames = int(round(max([e for _, e, _ in list(ref) + list(hyp)] or [0.0]) / DER_FRAME))
    r_names, h_names = {}, {}
    r, h = _frame_labels(ref, frames, r_names), _frame_labels(hyp, frames, h_names)
    speech = int((r >= 0).sum())
    if speech == 0:
        raise ValueError("der: the reference holds no speech")
    both = (r >= 0) & (h >= 0)
    overlap = np.zeros((max(len(r_names), 1), max(len(h_names), 1)), np.int64)
    np.add.at(overlap, (r[both], h[both]), 1)
    rows, cols = linear_sum_assignment(-overlap)
    miss = int(((r >= 0) & (h < 0)).sum())
    fa = int(((r < 0) & (h >= 0)).sum())
    conf = int(both.sum()) - int(overlap[rows, cols].sum())
    return miss / speech, fa / speech, conf / speech, (miss + fa + conf) / speech


def vbx_init(labels, num_speakers, smoothing=5.0):
    """The responsibilities VBx starts from: one-hot rows of the clusterer's labels times `smoothing`, a softmax per row (smoothing 5: 0.99
    on the labelled speaker of two, less with more speakers).  -> float32 [len(labels), num_speakers]; host arithmetic in double."""
    labels = np.asarray(labels, dtype=np.int64)
    num_speakers = int(num_speakers)
    if labels.ndim != 1 or labels.size == 0 or num_speakers < 1 or labels.min() < 0 or labels.max() >= num_speakers:
        raise ValueError("vbx_init: labels must be a non-empty 1-D array of values in 0 .. %d" % (num_speakers - 1))
    if not smoothing >= 0:
        raise ValueError("vbx_init: smoothing must not be negative (got %r)" % (smoothing,))
    z = np.zeros((labels.size, num_speakers), np.float64)
    z[np.arange(labels.size), labels] = float(smoothing)
    z = np.exp(z - z.max(axis=1, keepdims=True))
    return (z / z.sum(axis=1, keepdims=True)).astype(np.float32)


class VbxOptions(object):
    """What ops.vbx is run with behind the clusterer: the scaling factors fa and fb of the statistics, the probability loop_prob of staying
    with a speaker from one window to the next, at most max_iters iterations that stop once the ELBO gains less than epsilon, and the
    smoothing of vbx_init."""

    def __init__(self, fa=0.3, fb=17.0, loop_prob=0.99, max_iters=20, epsilon=1e-4, init_smoothing=5.0):
        self.fa, self.fb, self.loop_prob = float(fa), float(fb), float(loop_prob)
        self.max_iters, self.epsilon, self.init_smoothing = int(max_iters), float(epsilon), float(init_smoothing)


def _first_appearance(labels):
    """Labels renumbered 0, 1, ... by the first row of each: the clusterer's convention."""
    _, first, inverse = np.unique(labels, return_index=True, return_inverse=True)
    return np.argsort(np.argsort(first))[inverse].astype(np.int32)


class Diarizer(object):
    """Clusters the window embeddings of recordings behind a scorer (CosineScorer, or BackendScorer in either mode).

        diar = Diarizer(scorer, threshold=0.2)                      # merge while the best average score is >= the threshold
        diar = Diarizer(scorer, reco2num_spk={"rec1": 2, ...})      # or: merge down to the given number of speakers
        labels = diar.cluster({"rec1": matrix1, ...})               # {recording: int32 labels, one per row}

        diar = Diarizer(scorer, threshold=0.0, vbx=VbxOptions())    # ... and VBx behind the clusterer (a BackendScorer in the plda mode)
        diar = Diarizer(scorer, threshold=0.0, target_energy=0.9)   # ... the recipe's per-recording PCA in front of the PLDA scores (plda mode)

    cluster() runs prepare -> dense per recording into one packed buffer of score matrices and one ops.ahc_cluster call over them, in
    batches such that the buffer and the clusterer's scratch of a call stay under the scorer's workspace_bytes.  With vbx the clusterer
    should stop early (too many speakers rather than too few): its labels give vbx_init's responsibilities, the windows go through the
    scorer's plda_space, and one ops.vbx call per batch re-assigns them and drops redundant speakers; the surviving speakers are numbered
    0, 1, ... by their first window.  A recording the clusterer leaves with more than 32 clusters is clustered once more down to 32.
    After cluster(), vbx_report holds per recording (speakers before, speakers after, iterations, last ELBO).
    With target_energy (None, or within 0.001 of 1: off, every result bit-identical) a batch goes through the scorer's prepare_pca - one
    ops.backend_pca_plda call - and each recording is scored with its own model; a recording whose PCA gives none (a single window, a zero
    covariance: p = 0) is scored with the global model.  VBx keeps running in the unreduced plda_space.  After cluster(), pca_report holds
    per recording the kept dimension p (0: the global model).
    first_pass_max_points (2 .. 2048; agglomerative-cluster's option and default): a recording of at most that many windows is clustered
    as ever, bit for bit; a longer one, up to 32768 windows, in two passes (ops.ahc_cluster_two_pass: contiguous subsets down to ten times
    the wanted clusters, then the survivors against each other) - both kinds may meet in one cluster() call.  xv_vbx and
    xv_backend_pca_plda keep their cap: vbx or target_energy with a recording of more than 2048 windows is refused by name."""

    def __init__(self, scorer, threshold=None, reco2num_spk=None, vbx=None, target_energy=None, first_pass_max_points=2048):
        if (threshold is None) == (reco2num_spk is None):
            raise ValueError("Diarizer: exactly one of threshold and reco2num_spk says when the merging stops")
        if vbx is not None and not hasattr(scorer, "plda_space"):
            raise ValueError("Diarizer: VBx needs a BackendScorer in the plda mode (its PLDA space), not %s" % type(scorer).__name__)
        if target_energy is not None:
            if getattr(scorer, "mode", None) != "plda" or not hasattr(scorer, "prepare_pca"):
                raise ValueError("Diarizer: target_energy (the per-recording PCA of PLDA scoring) needs a BackendScorer in the plda mode, not %s%s"
                                 % (type(scorer).__name__, " in the %s mode" % scorer.mode if hasattr(scorer, "mode") else ""))
            target_energy = float(target_energy)
            if not 0.0 < target_energy <= 1.0:
                raise ValueError("Diarizer: target_energy must lie in (0, 1] (got %r)" % (target_energy,))
            if target_energy > 1.0 - 0.001:      # (ivector-plda-scoring-dense returns early: no PCA at all)
                target_energy = None
        self.target_energy, self.pca_report = target_energy, {}
        self.scorer, self.threshold, self.reco2num_spk, self.vbx = scorer, threshold, reco2num_spk, vbx
        self.torch, self.ops = scorer.torch, scorer.ops
        self.vbx_report = {}
        self.first_pass_max_points = int(first_pass_max_points)
        if not 2 <= self.first_pass_max_points <= FIRST_PASS_CAP:
            raise ValueError("Diarizer: first_pass_max_points must lie in 2 .. %d (got %r)" % (FIRST_PASS_CAP, first_pass_max_points))

    def _ahc(self, packed, offsets, n, ld, targets, names):
        """The clusterer over one batch -> the labels back to back.  The recordings of at most first_pass_max_points windows go through one
        ops.ahc_cluster call; the longer ones through ops.ahc_cluster_two_pass, one call per stop rule (by threshold, by target)."""
        threshold = 0.0 if self.threshold is None else float(self.threshold)
        long = n > self.first_pass_max_points
        if not long.any():
            return self.ops.ahc_cluster(packed, offsets, n.astype(np.int32), ld.astype(np.int32), threshold=threshold,
                                        targets=targets.astype(np.int32))[0].cpu().numpy()
        at = np.concatenate([[0], np.cumsum(n)])
        labels = np.empty(int(at[-1]), np.int32)
        for pick, by_target in ((~long, None), (long & (targets == 0), False), (long & (targets > 0), True)):
            idx = np.flatnonzero(pick)
            if idx.size == 0:
                continue
            if by_target is None:
                got = self.ops.ahc_cluster(packed, offsets[idx], n[idx].astype(np.int32), ld[idx].astype(np.int32), threshold=threshold,
                                           targets=targets[idx].astype(np.int32))[0]
            else:
                try:
                    got = self.ops.ahc_cluster_two_pass(packed, offsets[idx], n[idx], ld[idx], threshold=threshold,
                                                        targets=targets[idx] if by_target else None, first_pass_max_points=self.first_pass_max_points)[0]
                except ValueError as e:
                    if not hasattr(e, "recording"):
                        raise
                    raise ValueError("Diarizer: recording %s: %s" % (names[idx[e.recording]], e.what))
            got = got.cpu().numpy()
            for j, lo in zip(idx, np.concatenate([[0], np.cumsum(n[idx])])):
                labels[at[j]:at[j + 1]] = got[lo:lo + n[j]]
        return labels

    def _two_pass_bytes(self, rows, ld, target):
        """What a recording of more than first_pass_max_points windows costs a batch: its matrix, the first pass's copies of the subsets, the
        scratch of the cluster sums and the seed - for the most clusters the first pass can leave (with a target: ten times the target per
        subset; by threshold: every window, up to the second pass's cap)."""
        subsets = np.diff(self.ops.ahc_subsets(rows, self.first_pass_max_points))
        survivors = int(np.minimum(subsets, 10 * target).sum()) if target > 0 else int(rows)
        survivors = min(survivors, self.ops.AHC_MAX_N)
        return int(4 * rows * ld + 4 * (subsets * subsets).sum() + self.ops.ahc_cluster_sums_workspace_bytes([rows], [survivors]) + 4 * survivors * survivors)

    def _vbx(self, names, matrices, labels, n):
        """ops.vbx over one batch: labels = the clusterer's, back to back.  -> the new labels, back to back."""
        opt, ops, torch = self.vbx, self.ops, self.torch
        at = np.concatenate([[0], np.cumsum(n)])
        rows, psi = zip(*(self.scorer.plda_space(m) for m in matrices))
        dim, ld = int(psi[0].numel()), int(rows[0].shape[1])
        speakers = np.asarray([int(labels[at[j]:at[j + 1]].max()) + 1 for j in range(len(names))], np.int64)
        gamma = np.concatenate([vbx_init(labels[at[j]:at[j + 1]], speakers[j], opt.init_smoothing).ravel() for j in range(len(names))])
        pi = np.concatenate([np.full(k, 1.0 / k, np.float32) for k in speakers])
        x = torch.cat([r.reshape(-1) for r in rows]) if len(rows) > 1 else rows[0].reshape(-1)
        dev = x.device
        gamma_d, _, elbo, n_iters, new = ops.vbx(x, at[:-1] * ld, n, dim, psi[0], torch.from_numpy(gamma).to(dev), torch.from_numpy(pi).to(dev), speakers,
                                                 ld=np.full(len(names), ld, np.int64), loop_prob=opt.loop_prob, fa=opt.fa, fb=opt.fb,
                                                 max_iters=opt.max_iters, epsilon=opt.epsilon)
        new, elbo, n_iters = new.cpu().numpy(), elbo.cpu().numpy(), n_iters.cpu().numpy()
        out = np.empty_like(new)
        for j, name in enumerate(names):
            if n_iters[j] < 1:
                raise RuntimeError("Diarizer: xv_vbx skipped recording %s (n_iters = %d)" % (name, int(n_iters[j])))
            out[at[j]:at[j + 1]] = _first_appearance(new[at[j]:at[j + 1]])
            self.vbx_report[name] = (int(speakers[j]), int(out[at[j]:at[j + 1]].max()) + 1, int(n_iters[j]), float(elbo[j, n_iters[j] - 1]))
        return out

    def cluster(self, embeddings):
        """embeddings: {recording: float32 [n, d] matrix} (host or device).  -> {recording: NumPy int32 [n]} in the mapping's order."""
        keys = list(embeddings)
        if not keys:
            return {}
        try:      # (here, not at load time: the host side of this module needs NumPy only)
            from .._host import greedy_batches, pitch4
        except (ImportError, ValueError):
            from _host import greedy_batches, pitch4
        n = np.asarray([int(embeddings[k].shape[0]) for k in keys], np.int64)
        for k, rows in zip(keys, n):
            if rows < 1 or rows > self.ops.AHC_MAX_POINTS:
                raise ValueError("Diarizer: recording %s has %d windows, 1 .. %d are taken" % (k, rows, self.ops.AHC_MAX_POINTS))
            for option, op, on in (("vbx", "xv_vbx", self.vbx is not None), ("target_energy", "xv_backend_pca_plda", self.target_energy is not None)):
                if on and rows > self.ops.AHC_MAX_N:
                    raise ValueError("Diarizer: recording %s has %d windows: %s= takes recordings of at most %d (%s keeps its cap; the two-pass "
                                     "clustering alone goes further)" % (k, rows, option, self.ops.AHC_MAX_N, op))
        if self.reco2num_spk is not None:
            missing = [k for k in keys if k not in self.reco2num_spk]
            if missing:
                raise ValueError("Diarizer: no number of speakers for recording %s" % missing[0])
            targets = np.asarray([int(self.reco2num_spk[k]) for k in keys], np.int64)
            if targets.min() < 1:
                raise ValueError("Diarizer: recording %s: the number of speakers must be positive" % keys[int(np.argmin(targets))])
            targets = np.minimum(targets, n)      # (fewer windows than speakers: every window its own cluster)
        else:
            targets = np.zeros(len(keys), np.int64)
        ld = np.asarray([pitch4(int(r)) for r in n], np.int64)
        cost = 4 * (n * ld + n * n)      # bytes of a recording: its matrix in the packed buffer and the clusterer's copy
        for i in np.flatnonzero(n > self.first_pass_max_points):
            cost[i] = self._two_pass_bytes(int(n[i]), int(ld[i]), int(targets[i]))
        if self.target_energy is not None:      # ... its unit-length rows packed for the op, the op's scratch and its fp32 outputs
            dim4 = pitch4(self.scorer.dim)
            cost = cost + 4 * n * dim4 + self.ops.backend_pca_plda_workspace_bytes(1, self.scorer.dim) + 4 * dim4 * (dim4 + 8)
            self.pca_report = {}
        if self.vbx is not None:         # (VBx runs once the clusterer's buffers are gone: a batch must hold the larger of the two)
            cap_s, dim4 = self.ops.VBX_MAX_SPEAKERS, pitch4(self.scorer.dim)
            cost = np.maximum(cost, np.asarray([4 * r * dim4 + 8 * r * cap_s + self.ops.vbx_workspace_bytes([r], [cap_s], self.scorer.dim) for r in n], np.int64))
            self.vbx_report = {}
        out = {}
        batches = greedy_batches(len(keys), lambda i, total=0: (total + int(cost[i]),), lambda total: total, self.scorer.workspace_bytes,
                                 too_big=lambda i, c: "Diarizer: recording %s needs %d bytes of scores, the workspace holds %d"
                                 % (keys[i], c, self.scorer.workspace_bytes))
        for batch in batches:
            offsets = np.concatenate([[0], np.cumsum(n[batch] * ld[batch])]).astype(np.int64)
            packed = self.torch.empty(int(offsets[-1]), dtype=self.torch.float32, device=self.scorer.device)
            own = None if self.target_energy is None else self.scorer.prepare_pca([embeddings[keys[i]] for i in batch], self.target_energy)
            for j, i in enumerate(batch):
                view = packed[int(offsets[j]):int(offsets[j + 1])].view(int(n[i]), int(ld[i]))[:, :int(n[i])]
                if own is None:
                    self.scorer.dense(self.scorer.prepare(embeddings[keys[i]]), out=view)
                else:
                    prepared, model = own[j]
                    self.pca_report[keys[i]] = 0 if model is None else int(model[0])
                    self.scorer.dense(prepared, out=view, model=model)
            del own
            labels = self._ahc(packed, offsets[:-1], n[batch], ld[batch], targets[batch], [keys[i] for i in batch])
            at = np.concatenate([[0], np.cumsum(n[batch])])
            if self.vbx is not None:
                cap = self.ops.VBX_MAX_SPEAKERS
                many = [j for j in range(len(batch)) if labels[at[j]:at[j + 1]].max() >= cap]
                if many:      # the clusterer once more, down to the most speakers VBx takes, for the batch as it stands
                    _LOG.info("[INFO] Recording %s: more than %d clusters, clustered once more down to %d for VBx."
                              % (", ".join(keys[batch[j]] for j in many), cap, cap))
                    again = targets[batch].copy()
                    again[many] = cap
                    relabel = self._ahc(packed, offsets[:-1], n[batch], ld[batch], again, [keys[i] for i in batch])
                    for j in many:
                        labels[at[j]:at[j + 1]] = relabel[at[j]:at[j + 1]]
                del packed
                labels = self._vbx([keys[i] for i in batch], [embeddings[keys[i]] for i in batch], labels, n[batch])
            for j, i in enumerate(batch):
                out[keys[i]] = labels[at[j]:at[j + 1]]
        return out
