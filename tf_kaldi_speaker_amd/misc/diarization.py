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
Tuning the threshold on a development set (nnet/lib/tune_diarization.py): Diarizer.sweep gives the labels of every
threshold from one clustering (the merge log and its cuts, ops.ahc_cut); reference_frames and frame_windows put a reference RTTM - with a
collar, and one of three rules for overlapped speech - and the windows on 10 ms frames; DerSweep counts the errors of every (recording,
threshold) on the device (ops.diar_confusion) and pools the DER: md-eval restated from its definition, not compared with a run of it.
Not here: unsupervised threshold calibration, overlap detection, UEM files, VBx or the per-recording PCA on
recordings of more than 2048 windows.
"""
import collections
import logging

import numpy as np

try:      # (_lib imports neither torch nor NumPy: the caps are read without a device library)
    from .. import _lib
except (ImportError, ValueError):
    import _lib

_LOG = logging.getLogger("tf_kaldi_speaker_amd")
DER_FRAME = 0.01      # seconds per frame of der()
FIRST_PASS_CAP = _lib.AHC_MAX_N      # the most windows a subset of the first pass may hold: the clusterer's cap


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


def _midpoint_cut(subsegs):
    """The windows sorted by start; where two consecutive ones overlap, the first ends and the second starts at the midpoint of the overlap.
    -> [[start, end, the window's index in subsegs]]."""
    order = sorted(range(len(subsegs)), key=lambda i: (subsegs[i][0], subsegs[i][1]))
    cut = [[float(subsegs[i][0]), float(subsegs[i][1]), i] for i in order]
    for a, b in zip(cut[:-1], cut[1:]):
        if a[1] > b[0]:
            a[1] = b[0] = 0.5 * (a[1] + b[0])
    return cut


def rttm_turns(subsegs, labels):
    """Speaker turns from clustered windows: subsegs [(start, end)] (any unit), labels one per window.  The windows are sorted by start;
    where two consecutive windows overlap, the first ends and the second starts at the midpoint of the overlap; then abutting windows of
    one label are merged.  -> list of (start, end, label)."""
    if len(subsegs) != len(labels):
        raise ValueError("rttm_turns: %d windows, %d labels" % (len(subsegs), len(labels)))
    turns = []
    for s, e, i in _midpoint_cut(subsegs):
        l = int(labels[i])
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


OVERLAP_RULES = ("score", "ignore", "first")      # what reference_frames does where reference turns overlap


def popcount32(x):      # the set bits of each uint32 of an array -> int64
    x = np.asarray(x, np.uint32).astype(np.int64)
    x = x - ((x >> 1) & 0x55555555)
    x = (x & 0x33333333) + ((x >> 2) & 0x33333333)
    return (((x + (x >> 4)) & 0x0F0F0F0F) * 0x01010101 & 0xFFFFFFFF) >> 24


def _frame(t):      # the 10 ms frame of a boundary at t seconds, not below 0 (as _frame_labels places it)
    return max(int(round(t / DER_FRAME)), 0)


def reference_frames(turns, frames, collar=0.0, overlap="score"):
    """The reference of one recording on its `frames` 10 ms frames, as md-eval sees it (restated from its definition, not compared with a
    run of it): turns [(start, end, speaker)] in seconds, a boundary at t being frame int(round(t / DER_FRAME)).  collar (seconds, md-eval's
    -c): with C = int(round(collar / DER_FRAME)) the frames q - C <= f < q + C around every start and end q of every turn are not scored.
    overlap: "score" - every reference speaker of a frame counts; "ignore" (md-eval's -1) - frames with two or more reference speakers are
    not scored; "first" - der()'s rule: the turn that starts first owns the frame.  Speakers are numbered in the order of their first turn.
    -> (ref_mask uint32 [frames]: bit s set if speaker s talks, scored uint8 [frames], the speakers' names); more than 32 speakers are refused."""
    if overlap not in OVERLAP_RULES:
        raise ValueError("reference_frames: overlap must be one of %s (got %r)" % (", ".join(OVERLAP_RULES), overlap))
    if not collar >= 0.0:
        raise ValueError("reference_frames: the collar must not be negative (got %r)" % (collar,))
    frames, c = int(frames), int(round(collar / DER_FRAME))
    mask, scored, names = np.zeros(frames, np.uint32), np.ones(frames, np.uint8), {}
    for s, e, l in sorted(turns, key=lambda t: (t[0], t[1])):
        k = names.setdefault(l, len(names))
        if k >= _lib.DIAR_MAX_SPEAKERS:
            raise ValueError("reference_frames: more than %d reference speakers in a recording (%s is one too many)" % (_lib.DIAR_MAX_SPEAKERS, l))
        span = mask[_frame(s):_frame(e)]
        if overlap == "first":
            span[span == 0] = np.uint32(1 << k)
        else:
            span |= np.uint32(1 << k)
        for q in (int(round(s / DER_FRAME)), int(round(e / DER_FRAME))):
            scored[max(q - c, 0):max(q + c, 0)] = 0
    if overlap == "ignore":
        scored[popcount32(mask) >= 2] = 0
    return mask, scored, list(names)


def frame_windows(subsegs, frames):
    """The window that owns each of a recording's `frames` 10 ms frames under rttm_turns' midpoint rule: subsegs [(start, end)] in seconds;
    a frame between two windows' boundaries (placed as reference_frames places them) belongs to that window, where two still overlap to
    the one that starts first (der()'s rule), and -1 says none.  It does not depend on the labels: once per recording.  -> int32 [frames]."""
    own = np.full(int(frames), -1, np.int32)
    for s, e, i in reversed(_midpoint_cut(subsegs)):
        own[_frame(s):_frame(e)] = i
    return own


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


# One batch of Diarizer.cluster: keys, windows n, pitches ld, targets [b]; offsets / bounds [b + 1]: where recording j's score matrix lies in the packed buffer / its labels back to back
_Batch = collections.namedtuple("_Batch", "keys n ld targets offsets bounds")


class Diarizer(object):
    """Clusters the window embeddings of recordings behind a scorer (CosineScorer, or BackendScorer in either mode).

        diar = Diarizer(scorer, threshold=0.2)                      # merge while the best average score is >= the threshold
        diar = Diarizer(scorer, reco2num_spk={"rec1": 2, ...})      # or: merge down to the given number of speakers
        labels = diar.cluster({"rec1": matrix1, ...})               # {recording: int32 labels, one per row}
        labels = diar.sweep({"rec1": matrix1, ...}, [0.1, 0.2])     # {recording: int32 [thresholds, rows]}: cluster() at every threshold, one clustering

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

    def __init__(self, scorer, threshold=None, reco2num_spk=None, vbx=None, target_energy=None, first_pass_max_points=FIRST_PASS_CAP):
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
        self.target_energy, self.pca_report, self.vbx_report = target_energy, {}, {}
        self.scorer, self.threshold, self.reco2num_spk, self.vbx = scorer, threshold, reco2num_spk, vbx
        try:      # (here, not at load time: the host side of this module needs NumPy only)
            from .. import _host
        except (ImportError, ValueError):
            import _host
        self.torch, self.ops, self.host = scorer.torch, scorer.ops, _host
        self.first_pass_max_points = int(first_pass_max_points)
        if not 2 <= self.first_pass_max_points <= FIRST_PASS_CAP:
            raise ValueError("Diarizer: first_pass_max_points must lie in 2 .. %d (got %r)" % (FIRST_PASS_CAP, first_pass_max_points))

    def cluster(self, embeddings):
        """embeddings: {recording: float32 [n, d] matrix} (host or device).  -> {recording: NumPy int32 [n]} in the mapping's order."""
        keys, host = list(embeddings), self.host
        if not keys:
            return {}
        n = self._windows(keys, embeddings)
        targets = self._targets(keys, n)
        ld = np.asarray([host.pitch4(int(r)) for r in n], np.int64)
        cost = self._bytes(n, ld, targets)
        self.pca_report, self.vbx_report, out = {}, {}, {}      # (the report of an option that is off stays empty)
        for picked in host.greedy_batches(len(keys), lambda i, total=0: (total + int(cost[i]),), lambda total: total, self.scorer.workspace_bytes,
                                          too_big=lambda i, c: "Diarizer: recording %s needs %d bytes of scores, the workspace holds %d"
                                          % (keys[i], c, self.scorer.workspace_bytes)):
            batch = _Batch([keys[i] for i in picked], n[picked], ld[picked], targets[picked], host.bounds(n[picked] * ld[picked]), host.bounds(n[picked]))
            matrices = [embeddings[k] for k in batch.keys]
            packed = self._scores(batch, matrices)
            labels = self._ahc(packed, batch, batch.targets)
            if self.vbx is not None:
                labels = self._at_most_vbx_speakers(packed, batch, labels)
                del packed      # (VBx runs once the clusterer's buffers are gone)
                labels = self._vbx(batch, matrices, labels)
            out.update((k, labels[lo:hi]) for k, lo, hi in zip(batch.keys, batch.bounds[:-1], batch.bounds[1:]))
        return out

    def sweep(self, embeddings, thresholds, vbx_grid=None):
        """The labels cluster() would give at each of `thresholds` (whatever stop rule this Diarizer was made with), label for label, at
        the cost of one clustering: the scores once per recording, as cluster() takes them (target_energy included); one ops.ahc_cluster
        call per batch with every target 1 - the full merge log - and one ops.ahc_cut call for all thresholds.  With vbx each cut's labels
        take cluster()'s route: max_clusters = 32 in the cut replaces the second clustering of a recording with more clusters than VBx
        takes, then ops.vbx per cut; vbx_grid (a list of VbxOptions) runs that for each entry in place of self.vbx.  A recording of more
        than first_pass_max_points windows has no single log: ops.ahc_cluster_two_pass once per threshold, and a log line says so.
        -> {recording: NumPy int32 [cuts, n]} in the mapping's order; with vbx_grid int32 [len(vbx_grid), cuts, n].  vbx_report holds the
        last cut's entries."""
        thresholds = np.asarray(thresholds, np.float64)
        if thresholds.ndim != 1 or thresholds.size == 0 or np.isnan(thresholds).any():
            raise ValueError("Diarizer: sweep takes a non-empty list of thresholds, none of them NaN")
        if vbx_grid is not None and (self.vbx is None or not len(vbx_grid)):
            raise ValueError("Diarizer: vbx_grid needs a Diarizer with vbx and at least one entry")
        keys, host = list(embeddings), self.host
        if not keys:
            return {}
        n = self._windows(keys, embeddings)
        ld = np.asarray([host.pitch4(int(r)) for r in n], np.int64)
        targets = np.zeros(len(keys), np.int64)
        cost = self._bytes(n, ld, targets) + 4 * thresholds.size * n      # (... and the labels of every cut)
        self.pca_report, self.vbx_report, out = {}, {}, {}
        for picked in host.greedy_batches(len(keys), lambda i, total=0: (total + int(cost[i]),), lambda total: total, self.scorer.workspace_bytes,
                                          too_big=lambda i, c: "Diarizer: recording %s needs %d bytes of scores, the workspace holds %d"
                                          % (keys[i], c, self.scorer.workspace_bytes)):
            batch = _Batch([keys[i] for i in picked], n[picked], ld[picked], targets[picked], host.bounds(n[picked] * ld[picked]), host.bounds(n[picked]))
            matrices = [embeddings[k] for k in batch.keys]
            packed = self._scores(batch, matrices)
            labels = self._ahc_cuts(packed, batch, thresholds)
            del packed
            if vbx_grid is not None:
                labels = np.stack([[self._vbx(batch, matrices, cut, opt) for cut in labels] for opt in vbx_grid])
            elif self.vbx is not None:
                labels = np.stack([self._vbx(batch, matrices, cut) for cut in labels])
            out.update((k, labels[..., lo:hi]) for k, lo, hi in zip(batch.keys, batch.bounds[:-1], batch.bounds[1:]))
        return out

    def _ahc_cuts(self, packed, batch, thresholds):
        """The clusterer's labels of one batch at every threshold -> int32 [cuts, windows of the batch]: the recordings of at most
        first_pass_max_points windows through one merge log and its cuts, the longer ones through the two passes, once per threshold."""
        ops, host, n = self.ops, self.host, batch.n
        long = n > self.first_pass_max_points
        labels = np.empty((thresholds.size, int(batch.bounds[-1])), np.int32)
        idx = np.flatnonzero(~long)
        if idx.size:
            _, merges, values, n_merges = ops.ahc_cluster(packed, batch.offsets[idx], n[idx], batch.ld[idx], targets=np.ones(idx.size, np.int64))
            cap = None if self.vbx is None else np.full(thresholds.size, _lib.VBX_MAX_SPEAKERS, np.int32)
            got, clusters = ops.ahc_cut(merges, values, n_merges, n[idx], thresholds, max_clusters=cap)
            skipped = clusters.min(dim=0)[0].cpu().numpy() < 1
            if skipped.any():
                raise RuntimeError("Diarizer: xv_ahc_cut skipped recording %s" % batch.keys[idx[int(np.argmax(skipped))]])
            got = got.cpu().numpy()
            for j, lo in zip(idx, host.bounds(n[idx])):
                labels[:, batch.bounds[j]:batch.bounds[j + 1]] = got[:, lo:lo + n[j]]
        idx = np.flatnonzero(long)
        if idx.size:
            _LOG.info("[INFO] Recording %s: more than %d windows, no single merge log: clustered in two passes once per threshold (%d times)."
                      % (", ".join(batch.keys[j] for j in idx), self.first_pass_max_points, thresholds.size))
            # the long recordings as a batch of their own on the same packed buffer (_ahc reads a matrix's start, not where it ends)
            own = _Batch([batch.keys[j] for j in idx], n[idx], batch.ld[idx], batch.targets[idx], np.append(batch.offsets[idx], batch.offsets[-1]), host.bounds(n[idx]))
            for k, threshold in enumerate(thresholds):
                one = self._ahc(packed, own, own.targets, threshold=float(threshold))
                if self.vbx is not None:
                    one = self._at_most_vbx_speakers(packed, own, one)
                for j, lo, hi in zip(idx, own.bounds[:-1], own.bounds[1:]):
                    labels[k, batch.bounds[j]:batch.bounds[j + 1]] = one[lo:hi]
        return labels

    def _windows(self, keys, embeddings):      # -> the windows of each recording; one that the clusterer, VBx or the PCA does not take is refused by name
        n = np.asarray([int(embeddings[k].shape[0]) for k in keys], np.int64)
        for k, rows in zip(keys, n):
            if rows < 1 or rows > _lib.AHC_MAX_POINTS:
                raise ValueError("Diarizer: recording %s has %d windows, 1 .. %d are taken" % (k, rows, _lib.AHC_MAX_POINTS))
            for option, op, cap, on in (("vbx", "xv_vbx", _lib.VBX_MAX_ROWS, self.vbx is not None),
                                        ("target_energy", "xv_backend_pca_plda", _lib.PCA_MAX_ROWS, self.target_energy is not None)):
                if on and rows > cap:
                    raise ValueError("Diarizer: recording %s has %d windows: %s= takes recordings of at most %d (%s keeps its cap; the two-pass "
                                     "clustering alone goes further)" % (k, rows, option, cap, op))
        return n

    def _targets(self, keys, n):      # -> the clusters each recording is merged down to (0: by the threshold)
        if self.reco2num_spk is None:
            return np.zeros(len(keys), np.int64)
        missing = [k for k in keys if k not in self.reco2num_spk]
        if missing:
            raise ValueError("Diarizer: no number of speakers for recording %s" % missing[0])
        targets = np.asarray([int(self.reco2num_spk[k]) for k in keys], np.int64)
        if targets.min() < 1:
            raise ValueError("Diarizer: recording %s: the number of speakers must be positive" % keys[int(np.argmin(targets))])
        return np.minimum(targets, n)      # (fewer windows than speakers: every window its own cluster)

    def _bytes(self, n, ld, targets):      # -> what each recording costs a batch, in bytes
        ops, pitch4 = self.ops, self.host.pitch4
        cost = 4 * (n * ld + n * n)      # its matrix in the packed buffer and the clusterer's copy
        for i in np.flatnonzero(n > self.first_pass_max_points):
            cost[i] = self._two_pass_bytes(int(n[i]), int(ld[i]), int(targets[i]))
        if self.target_energy is not None:      # ... its unit-length rows packed for the op, the op's scratch and its fp32 outputs
            dim4 = pitch4(self.scorer.dim)
            cost = cost + 4 * n * dim4 + ops.backend_pca_plda_workspace_bytes(1, self.scorer.dim) + 4 * dim4 * (dim4 + 8)
        if self.vbx is not None:         # (VBx runs once the clusterer's buffers are gone: a batch must hold the larger of the two)
            cap, dim4 = _lib.VBX_MAX_SPEAKERS, pitch4(self.scorer.dim)
            cost = np.maximum(cost, np.asarray([4 * r * dim4 + 8 * r * cap + ops.vbx_workspace_bytes([r], [cap], self.scorer.dim) for r in n], np.int64))
        return cost

    def _two_pass_bytes(self, rows, ld, target):
        """What a recording of more than first_pass_max_points windows costs a batch: its matrix, the first pass's copies of the subsets, the
        scratch of the cluster sums and the seed - for the most clusters the first pass can leave (with a target: ten times the target per
        subset; by threshold: every window, up to the second pass's cap)."""
        subsets = np.diff(self.ops.ahc_subsets(rows, self.first_pass_max_points))
        survivors = min(int(np.minimum(subsets, 10 * target).sum()) if target > 0 else int(rows), _lib.AHC_MAX_N)
        return int(4 * rows * ld + 4 * (subsets * subsets).sum() + self.ops.ahc_cluster_sums_workspace_bytes([rows], [survivors]) + 4 * survivors * survivors)

    def _scores(self, batch, matrices):      # prepare -> dense of every recording of the batch -> the packed buffer of their score matrices
        scorer, packed = self.scorer, self.torch.empty(int(batch.offsets[-1]), dtype=self.torch.float32, device=self.scorer.device)
        own = None if self.target_energy is None else scorer.prepare_pca(matrices, self.target_energy)
        for j, (key, matrix) in enumerate(zip(batch.keys, matrices)):
            rows = int(batch.n[j])
            view = packed[int(batch.offsets[j]):int(batch.offsets[j + 1])].view(rows, int(batch.ld[j]))[:, :rows]
            if own is None:
                scorer.dense(scorer.prepare(matrix), out=view)
            else:
                prepared, model = own[j]
                self.pca_report[key] = 0 if model is None else int(model[0])
                scorer.dense(prepared, out=view, model=model)
        return packed

    def _ahc(self, packed, batch, targets, threshold=None):
        """The clusterer over one batch -> the labels back to back.  The recordings of at most first_pass_max_points windows go through one
        ops.ahc_cluster call; the longer ones through ops.ahc_cluster_two_pass, one call per stop rule (by threshold, by target).
        threshold None: this Diarizer's."""
        ops, offsets, n, ld = self.ops, batch.offsets[:-1], batch.n, batch.ld
        if threshold is None:
            threshold = 0.0 if self.threshold is None else float(self.threshold)
        long = n > self.first_pass_max_points
        labels = np.empty(int(batch.bounds[-1]), np.int32)
        for pick, by_target in ((~long, None), (long & (targets == 0), False), (long & (targets > 0), True)):
            idx = np.flatnonzero(pick)
            if idx.size == 0:
                continue
            if by_target is None:
                got = ops.ahc_cluster(packed, offsets[idx], n[idx], ld[idx], threshold=threshold, targets=targets[idx])[0]
            else:
                try:
                    got = ops.ahc_cluster_two_pass(packed, offsets[idx], n[idx], ld[idx], threshold=threshold, targets=targets[idx] if by_target else None,
                                                   first_pass_max_points=self.first_pass_max_points)[0]
                except ops.TwoPassRefusal as e:
                    raise ValueError("Diarizer: recording %s: %s" % (batch.keys[idx[e.recording]], e.what))
            got = got.cpu().numpy()
            for j, lo in zip(idx, self.host.bounds(n[idx])):
                labels[batch.bounds[j]:batch.bounds[j + 1]] = got[lo:lo + n[j]]
        return labels

    def _at_most_vbx_speakers(self, packed, batch, labels):      # the clusterer once more where it left more speakers than VBx takes
        cap, at = _lib.VBX_MAX_SPEAKERS, batch.bounds
        many = np.asarray([labels[lo:hi].max() >= cap for lo, hi in zip(at[:-1], at[1:])])
        if many.any():      # ... down to that many, for the batch as it stands
            _LOG.info("[INFO] Recording %s: more than %d clusters, clustered once more down to %d for VBx." % (", ".join(np.asarray(batch.keys)[many]), cap, cap))
            relabel = self._ahc(packed, batch, np.where(many, cap, batch.targets))
            for j in np.flatnonzero(many):
                labels[at[j]:at[j + 1]] = relabel[at[j]:at[j + 1]]
        return labels

    def _vbx(self, batch, matrices, labels, opt=None):
        """ops.vbx over one batch: labels = the clusterer's, back to back; opt None: this Diarizer's options.  -> the new labels, back to back."""
        opt, torch, at = opt or self.vbx, self.torch, batch.bounds
        rows, psi = zip(*(self.scorer.plda_space(m) for m in matrices))
        x, offsets, n, ld = self.host.pack_rows(rows)
        dim, recordings = int(psi[0].numel()), range(len(batch.keys))
        speakers = np.asarray([int(labels[at[j]:at[j + 1]].max()) + 1 for j in recordings], np.int64)
        gamma = np.concatenate([vbx_init(labels[at[j]:at[j + 1]], speakers[j], opt.init_smoothing).ravel() for j in recordings])
        pi = np.concatenate([np.full(k, 1.0 / k, np.float32) for k in speakers])
        gamma_d, _, elbo, n_iters, new = self.ops.vbx(x, offsets, n, dim, psi[0], torch.from_numpy(gamma).to(x.device), torch.from_numpy(pi).to(x.device), speakers, ld=ld,
                                                      loop_prob=opt.loop_prob, fa=opt.fa, fb=opt.fb, max_iters=opt.max_iters, epsilon=opt.epsilon)
        new, elbo, n_iters = new.cpu().numpy(), elbo.cpu().numpy(), n_iters.cpu().numpy()
        out = np.empty_like(new)
        for j, name in enumerate(batch.keys):
            if n_iters[j] < 1:
                raise RuntimeError("Diarizer: xv_vbx skipped recording %s (n_iters = %d)" % (name, int(n_iters[j])))
            out[at[j]:at[j + 1]] = _first_appearance(new[at[j]:at[j + 1]])
            self.vbx_report[name] = (int(speakers[j]), int(out[at[j]:at[j + 1]].max()) + 1, int(n_iters[j]), float(elbo[j, n_iters[j] - 1]))
        return out


class DerSweep(object):
    """The diarization error of many label sets against one reference, counted on the device: md-eval's figures (-c collar, -1) restated
    from its definition - nothing is compared with a run of md-eval.

        sweep = DerSweep(device, {"rec1": ref_turns, ...}, {"rec1": [(start, end), ...], ...}, collar=0.25)     # seconds; once
        table = sweep.score(diarizer.sweep(embeddings, thresholds))                                            # any number of times

    The reference frames (reference_frames) and the owning windows (frame_windows) of every recording are built and uploaded once
    (ops.diar_frames); a recording has as many 10 ms frames as its last reference turn or window needs.  score(labels) takes
    {recording: int [cuts, n]} (one label per window and cut), runs one ops.diar_confusion call over all recordings and cuts, and maps
    the speakers of every (recording, cut) one to one such that the matched time over the scored frames is largest
    (scipy.optimize.linear_sum_assignment on the counted overlap, as der() does): speaker error = sum of min(reference speakers, [a
    hypothesis speaker]) - matched.  -> DerTable."""

    def __init__(self, device, reference, subsegs, collar=0.0, overlap="score"):
        try:
            from .. import _host
        except (ImportError, ValueError):
            import _host
        self.torch, self.ops, self.device = _host.device_ops(device)
        self.keys = list(reference)
        if set(self.keys) != set(subsegs):
            odd = sorted(set(self.keys) ^ set(subsegs))[0]
            raise ValueError("DerSweep: recording %s has %s" % (odd, "a reference but no windows" if odd in reference else "windows but no reference"))
        if not self.keys:
            raise ValueError("DerSweep: no recording")
        masks, flags, owners, self.names = [], [], [], {}
        for k in self.keys:
            frames = _frame(max([e for _, e, _ in reference[k]] + [e for _, e in subsegs[k]]))
            mask, scored, self.names[k] = reference_frames(reference[k], frames, collar, overlap)
            if not self.names[k]:
                raise ValueError("DerSweep: recording %s has no reference turn" % k)
            masks.append(mask), flags.append(scored), owners.append(frame_windows(subsegs[k], frames))
        self.n = np.asarray([len(subsegs[k]) for k in self.keys], np.int64)
        self.speakers = np.asarray([len(self.names[k]) for k in self.keys], np.int64)
        self.frames = self.ops.diar_frames(np.concatenate(masks), np.concatenate(flags), np.concatenate(owners), [m.size for m in masks], self.n,
                                           self.speakers, self.device)

    def score(self, labels):
        from scipy.optimize import linear_sum_assignment
        per = [np.asarray(labels[k]) for k in self.keys]
        for k, lab, n in zip(self.keys, per, self.n):
            if lab.ndim != 2 or lab.shape != (per[0].shape[0], n) or lab.dtype.kind not in "iu" or lab.shape[0] < 1 or lab.min() < 0:
                raise ValueError("DerSweep: recording %s: labels must be a non-negative integer [cuts, %d] array, the cuts of every recording alike" % (k, n))
        clusters = np.stack([lab.max(axis=1) + 1 for lab in per], axis=1)
        stacked = self.torch.from_numpy(np.ascontiguousarray(np.concatenate(per, axis=1), dtype=np.int32)).to(self.device)
        totals, overlap, offsets, status = self.ops.diar_confusion(self.frames, stacked, clusters)
        totals, overlap, status = totals.cpu().numpy(), overlap.cpu().numpy(), status.cpu().numpy()
        error = np.zeros(status.shape, np.int64)
        for k, i in zip(*np.nonzero(status == 0)):
            shared = overlap[offsets[k, i]:offsets[k, i] + self.speakers[i] * clusters[k, i]].reshape(self.speakers[i], clusters[k, i])
            rows, cols = linear_sum_assignment(-shared)
            error[k, i] = totals[k, i, 0] - totals[k, i, 1] - int(shared[rows, cols].sum())
        return DerTable(self.keys, totals[..., 0], totals[..., 1], totals[..., 2], error, status, clusters)


class DerTable(object):
    """DerSweep.score's counts in frames, int64 [cuts, recordings]: speech (scored reference speaker time), miss, fa (false alarm), error
    (speaker error); status int32 (ops.diar_confusion's: 0 counted) and clusters per (cut, recording).  pooled(k): cut k's (miss, false
    alarm, speaker error, DER) over all recordings - summed counts over summed scored speaker time, md-eval's overall figure - or None if a
    recording of the cut was not counted; why_not(k) then names the first such recording and the reason."""

    def __init__(self, keys, speech, miss, fa, error, status, clusters):
        self.keys, self.speech, self.miss, self.fa, self.error, self.status, self.clusters = keys, speech, miss, fa, error, status, clusters
        if int(speech[0].sum()) == 0:      # (the scored reference time does not depend on the cut)
            raise ValueError("DerSweep: the reference holds no scored speech")

    def pooled(self, k):
        if (self.status[k] != 0).any():
            return None
        speech, parts = int(self.speech[k].sum()), [int(c[k].sum()) for c in (self.miss, self.fa, self.error)]
        return tuple(p / speech for p in parts) + (sum(parts) / speech,)

    def why_not(self, k):
        i = int(np.argmax(self.status[k] != 0))
        if self.status[k, i] == 1:
            return "recording %s has %d clusters, %d are counted" % (self.keys[i], int(self.clusters[k, i]), _lib.DIAR_MAX_CLUSTERS)
        return "recording %s was skipped by xv_diar_confusion (status %d)" % (self.keys[i], int(self.status[k, i]))
