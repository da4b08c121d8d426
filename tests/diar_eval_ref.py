"""NumPy restatement of threshold tuning for diarization (include/xvector_hip.h: xv_ahc_cut, xv_diar_confusion; misc/diarization.py:
reference_frames, frame_windows, DerSweep): the cut rule on a merge log, the per-frame error counts, and the pooled error of hypothesis
turns against reference turns with a collar.  Everything here is integer arithmetic behind the comparisons of the cut rule, so the GPU
and the host code must agree with it exactly.  md-eval is restated from its definition; nothing is compared with a run of it."""
import numpy as np
from scipy.optimize import linear_sum_assignment

FRAME = 0.01


def cut(merges, values, n, threshold, min_clusters=1, max_clusters=None):
    """Labels of n rows after the leading entries of the log (merges [m][2], values float32 [m]) that cut (threshold, min_clusters,
    max_clusters) applies -> (labels int32 [n], clusters)."""
    values = np.asarray(values, np.float32)
    m, threshold = len(values), np.float32(threshold)
    p = 0
    while p < m and values[p] >= threshold:      # the first entry that fails ends it: the log need not be monotone
        p += 1
    p = min(max(min(p, n - min_clusters), 0), m)
    p = min(max(max(p, n - (n if max_clusters is None else max_clusters)), 0), m)
    member = [[i] for i in range(n)]      # replayed one merge after the other: b's members go to a
    for a, b in np.asarray(merges, np.int64).reshape(-1, 2)[:p]:
        member[a] += member[b]
        member[b] = []
    labels, next_label = np.empty(n, np.int32), 0
    for i in range(n):      # ascending smallest member
        if member[i]:
            labels[member[i]] = next_label
            next_label += 1
    return labels, next_label


def popcount(x):
    return np.asarray([bin(int(v)).count("1") for v in x], np.int64)


def confusion(ref_mask, scored, frame_window, labels, speakers, clusters):
    """(speech, miss, fa, overlap int64 [speakers][clusters]) over the scored frames; labels: one per window."""
    overlap = np.zeros((speakers, clusters), np.int64)
    on = np.flatnonzero(np.asarray(scored) != 0)
    ref, win = np.asarray(ref_mask, np.uint32)[on], np.asarray(frame_window, np.int64)[on]
    has = win >= 0
    h = np.where(has, np.asarray(labels, np.int64)[np.maximum(win, 0)], -1)
    pc = popcount(ref)
    for s in range(speakers):
        talks = ((ref >> np.uint32(s)) & np.uint32(1)).astype(bool) & has
        np.add.at(overlap[s], h[talks], 1)
    return int(pc.sum()), int(np.maximum(pc - has, 0).sum()), int(np.maximum(has.astype(np.int64) - pc, 0).sum()), overlap


def speaker_error(speech, miss, overlap):
    rows, cols = linear_sum_assignment(-overlap)
    return speech - miss - int(overlap[rows, cols].sum())


def frame_of(t):
    return int(round(t / FRAME))


def reference(turns, frames, collar=0.0, overlap="score"):
    """Frame by frame, from the definition: (mask, scored) of reference turns [(start, end, speaker)] in seconds."""
    names, spans = {}, []
    for s, e, l in sorted(turns, key=lambda t: (t[0], t[1])):
        spans.append((frame_of(s), frame_of(e), names.setdefault(l, len(names))))
    c = frame_of(collar)
    mask, scored = np.zeros(frames, np.uint32), np.ones(frames, np.uint8)
    for f in range(frames):
        who = [k for a, b, k in spans if a <= f < b]
        if overlap == "first":
            who = who[:1]
        for k in who:
            mask[f] |= np.uint32(1 << k)
        if any(q - c <= f < q + c for a, b, _ in spans for q in (a, b)) or (overlap == "ignore" and len(set(who)) >= 2):
            scored[f] = 0
    return mask, scored, len(names)


def hypothesis(turns, frames):
    """One hypothesis speaker per frame, -1 none: turns [(start, end, label)] in seconds; where two overlap, the one that starts first."""
    h = np.full(frames, -1, np.int64)
    for s, e, l in sorted(turns, key=lambda t: (t[0], t[1]), reverse=True):
        h[max(frame_of(s), 0):max(frame_of(e), 0)] = l
    return h


def der_counts(ref_turns, hyp_turns, frames, collar=0.0, overlap="score"):
    """(speech, miss, fa, speaker error) in frames of one recording: hyp_turns carry integer labels 0, 1, ..."""
    mask, scored, speakers = reference(ref_turns, frames, collar, overlap)
    h = hypothesis(hyp_turns, frames)
    clusters = int(h.max()) + 1 if h.size and h.max() >= 0 else 1
    # (a frame's hypothesis speaker as the label of a window of its own: frame_window = the frame, -1 without a speaker)
    speech, miss, fa, shared = confusion(mask, scored, np.where(h >= 0, np.arange(frames), -1), np.maximum(h, 0), max(speakers, 1), clusters)
    return speech, miss, fa, speaker_error(speech, miss, shared)
