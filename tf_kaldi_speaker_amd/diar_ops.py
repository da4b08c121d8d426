"""Op-level wrappers of the diarization kernels (include/xvector_hip.h): the ops that take the recordings of one call as ragged arrays in
one 1-D float32 buffer - the agglomerative clusterers, the cluster sums of the two-pass clustering and the cuts of a merge log
(csrc/xv_ahc.hip), VBx (csrc/xv_vbx.hip) and the per-recording PCA of PLDA scoring (csrc/xv_backend_pca.hip) - and the error counts of
diarization scoring (csrc/xv_diar_eval.hip); the dense scores they cluster are pipeline_ops.py's.  ops.py re-exports
every public name here: callers write ops.ahc_cluster.  The kernels trust their index arrays: _host.recordings checks them before the upload."""
import collections
import ctypes as C

import numpy as np
import torch

try:
    from ._host import _lib, _p, _s, bounds, cluster_outputs, exclusive_offsets, f32_values, host_ints, pitch4, recordings, upload
except ImportError:
    from _host import _lib, _p, _s, bounds, cluster_outputs, exclusive_offsets, f32_values, host_ints, pitch4, recordings, upload

AHC_MAX_N, AHC_MAX_POINTS, PCA_MAX_ROWS, PCA_MAX_DIM = _lib.AHC_MAX_N, _lib.AHC_MAX_POINTS, _lib.PCA_MAX_ROWS, _lib.PCA_MAX_DIM      # (_lib.py says what each one caps)
VBX_MAX_ROWS, VBX_MAX_SPEAKERS, VBX_MAX_DIM, VBX_MAX_ITERS = _lib.VBX_MAX_ROWS, _lib.VBX_MAX_SPEAKERS, _lib.VBX_MAX_DIM, _lib.VBX_MAX_ITERS
DIAR_MAX_SPEAKERS, DIAR_MAX_CLUSTERS = _lib.DIAR_MAX_SPEAKERS, _lib.DIAR_MAX_CLUSTERS


def ahc_workspace_bytes(n):
    """Bytes of scratch xv_ahc_cluster needs for recordings of n[i] rows (a host integer array): every recording's n x n matrix."""
    n = np.asarray(n, dtype=np.int64)
    return int(_lib.load().xv_ahc_workspace_bytes(C.c_int64(int((n * n).sum()))))


def ahc_cluster(scores, mat_offsets, n, ld=None, threshold=0.0, targets=None):
    """Average-linkage agglomerative clustering of b score matrices in one call (xv_ahc_cluster; include/xvector_hip.h states the arithmetic,
    tests/ahc_ref.py restates it).  scores: a contiguous 1-D float32 device buffer; recording i's matrix [n[i], ld[i]] starts at float
    mat_offsets[i] and only its upper triangle is read.  targets[i] = 0 (None: all 0): merge while the best average score is >= threshold;
    t >= 1: merge down to t clusters, whatever the scores.  mat_offsets, n, ld (None: n), targets: HOST integer arrays, checked here before
    the upload - the kernel trusts them.  -> (labels int32 [sum n], merges int32 [sum (n - 1), 2], merge_values float32 [sum (n - 1)],
    n_merges int32 [b]), device tensors; recording i's labels start at the exclusive prefix of n, its merge log at that of n - 1 and holds
    n_merges[i] entries.  A NaN score is undefined."""
    n, ld, mat_offsets = recordings("ahc_cluster", scores, mat_offsets, n, ld, AHC_MAX_N)
    b = n.size
    targets = np.zeros(b, np.int32) if targets is None else host_ints(targets, "ahc_cluster: targets", n=b)
    if (targets < 0).any() or (targets > n).any():
        i = int(np.argmax((targets < 0) | (targets > n)))
        raise ValueError("ahc_cluster: recording %d: target %d outside 0 .. %d" % (i, int(targets[i]), int(n[i])))
    dev = scores.device
    written, out = cluster_outputs(n, dev)
    ws_bytes = ahc_workspace_bytes(n)
    ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=dev)
    off_d, n_d, ld_d, t_d = upload(mat_offsets, np.int64, dev), upload(n, np.int32, dev), upload(ld, np.int32, dev), upload(targets, np.int32, dev)
    _lib.call("xv_ahc_cluster", _s(), _p(scores), C.c_int64(scores.numel()), _p(off_d), _p(n_d), _p(ld_d), _p(t_d), b, int(n.max()), C.c_int64(int(n.sum())),
              C.c_int64(int((n * n).sum())), C.c_float(float(threshold)), *[_p(t) for t in written], _p(ws), C.c_size_t(ws_bytes))
    return out


def ahc_cluster_from(scores, mat_offsets, n, ld=None, floors=None, threshold=float("-inf"), seed=None, sizes=None):
    """The clusterer with a floor (xv_ahc_cluster_from; tests/ahc2_ref.py restates it): recording i merges while it has more than floors[i]
    clusters (1 .. n[i]; None: 1) AND the best average score is >= threshold (-inf: down to the floor).  Two starts.  From scores (seed
    None): scores, mat_offsets, n, ld as for ahc_cluster - a sub-block of a matrix is a matrix at an offset on that matrix's pitch.
    Seeded: seed is a contiguous 1-D float32 device tensor that holds recording i's T [n[i], n[i]] (symmetric, pitch n[i]) at the exclusive
    prefix of n^2 - it is the clusterer's scratch and is MODIFIED -, sizes a HOST integer array [sum n], each >= 1, a recording's together at
    most 32768 (ahc_cluster_sums gives both); scores, mat_offsets and ld must be None.  -> ahc_cluster's four outputs."""
    name = "ahc_cluster_from"
    if seed is None:
        if sizes is not None:
            raise ValueError("%s: sizes belong to a seeded start (seed is None)" % name)
        n, ld, mat_offsets = recordings(name, scores, mat_offsets, n, ld, AHC_MAX_N)
        dev = scores.device
    else:
        if scores is not None or mat_offsets is not None or ld is not None:
            raise ValueError("%s: a seeded start reads no scores (scores, mat_offsets and ld must be None)" % name)
        n = host_ints(n, name + ": n", min_size=1, dtype=np.int64)
        if n.min() < 1 or n.max() > AHC_MAX_N:
            i = int(np.argmax((n < 1) | (n > AHC_MAX_N)))
            raise ValueError("%s: recording %d has %d clusters, 1 .. %d are taken" % (name, i, int(n[i]), AHC_MAX_N))
        if seed.dtype != torch.float32 or seed.dim() != 1 or not seed.is_contiguous() or seed.numel() < int((n * n).sum()):
            raise ValueError("%s: seed must be a contiguous 1-D float32 tensor of at least %d floats" % (name, int((n * n).sum())))
        sizes = host_ints(sizes if sizes is not None else [], name + ": sizes", n=int(n.sum()))
        members = np.add.reduceat(np.maximum(sizes, 0).astype(np.int64), exclusive_offsets(n))
        wrong = (np.minimum.reduceat(sizes, exclusive_offsets(n)) < 1) | (members > AHC_MAX_POINTS)
        if wrong.any():
            raise ValueError("%s: recording %d: the sizes must be positive and add up to at most %d" % (name, int(np.argmax(wrong)), AHC_MAX_POINTS))
        dev = seed.device
    b = n.size
    floors = np.ones(b, np.int32) if floors is None else host_ints(floors, name + ": floors", n=b)
    if (floors < 1).any() or (floors > n).any():
        i = int(np.argmax((floors < 1) | (floors > n)))
        raise ValueError("%s: recording %d: floor %d outside 1 .. %d" % (name, i, int(floors[i]), int(n[i])))
    threshold = float(threshold)
    if threshold != threshold:
        raise ValueError("%s: the threshold is NaN" % name)
    sum_n2 = int((n * n).sum())
    written, out = cluster_outputs(n, dev)
    n_d, f_d = upload(n, np.int32, dev), upload(floors, np.int32, dev)
    if seed is None:
        ws_bytes = int(_lib.load().xv_ahc_cluster_from_workspace_bytes(C.c_int64(sum_n2)))
        ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=dev)
        off_d, ld_d, s_d = upload(mat_offsets, np.int64, dev), upload(ld, np.int32, dev), None
    else:
        ws, ws_bytes, off_d, ld_d, s_d = seed, seed.numel() * 4, None, None, upload(sizes, np.int32, dev)
    _lib.call("xv_ahc_cluster_from", _s(), _p(scores), C.c_int64(scores.numel() if scores is not None else 0), _p(off_d), _p(n_d), _p(ld_d), _p(f_d),
              _p(s_d), int(seed is not None), b, int(n.max()), C.c_int64(int(n.sum())), C.c_int64(sum_n2), C.c_float(threshold), *[_p(t) for t in written],
              _p(ws), C.c_size_t(ws_bytes))
    return out


def ahc_member_lists(labels, n):
    """Clusters as the member lists ahc_cluster_sums takes, from HOST labels [sum n] (recording i's n[i] back to back, numbered 0, 1, ... in
    the order of their smallest members, as the clusterer numbers them).  -> (members int32 [sum n], starts int32 [sum (c + 1)], c int64 [b])."""
    n = host_ints(n, "ahc_member_lists: n", min_size=1, dtype=np.int64)
    labels = host_ints(labels, "ahc_member_lists: labels", n=int(n.sum()))
    members, starts, c = [], [], []
    for lab in np.split(labels, bounds(n)[1:-1]):
        uniq, first = np.unique(lab, return_index=True)
        if lab.size == 0 or uniq[0] != 0 or uniq[-1] != uniq.size - 1 or (np.diff(first) <= 0).any():
            raise ValueError("ahc_member_lists: a recording's labels must be 0, 1, ... in the order of the clusters' smallest members")
        members.append(np.argsort(lab, kind="stable").astype(np.int32))
        starts.append(bounds(np.bincount(lab)).astype(np.int32))
        c.append(uniq.size)
    return np.concatenate(members), np.concatenate(starts), np.asarray(c, np.int64)


def ahc_cluster_sums_workspace_bytes(n, c):
    """Bytes of scratch xv_ahc_cluster_sums needs for recordings of n[i] rows in c[i] clusters (host integer arrays of one length)."""
    n, c = np.asarray(n, dtype=np.int64), np.asarray(c, dtype=np.int64)
    return int(_lib.load().xv_ahc_cluster_sums_workspace_bytes(int(n.size), C.c_int64(int((n * c).sum()))))


def ahc_cluster_sums(scores, mat_offsets, n, ld, members, starts, c):
    """The seed of a second clustering pass (xv_ahc_cluster_sums; include/xvector_hip.h states the order of every sum, tests/ahc2_ref.py
    restates it): T[A][B] = the sum of the scores between the members of clusters A and B of each of b recordings, from the upper triangles
    of their matrices (scores, mat_offsets, n <= 32768, ld as for ahc_cluster).  members, starts, c: HOST integer arrays as ahc_member_lists
    gives them - recording i's rows cluster by cluster, clusters ascending by smallest member, members ascending; c[i] <= 2048 - checked
    here before the upload.  -> (seed float32 [sum c^2], sizes int32 [sum c]), device tensors: what ahc_cluster_from takes for a seeded start."""
    name = "ahc_cluster_sums"
    n, ld, mat_offsets = recordings(name, scores, mat_offsets, n, ld, AHC_MAX_POINTS)
    b = n.size
    c = host_ints(c, name + ": c", n=b, dtype=np.int64)
    if (c < 1).any() or (c > np.minimum(n, AHC_MAX_N)).any():
        i = int(np.argmax((c < 1) | (c > np.minimum(n, AHC_MAX_N))))
        raise ValueError("%s: recording %d has %d clusters, 1 .. %d are taken" % (name, i, int(c[i]), int(min(n[i], AHC_MAX_N))))
    members = host_ints(members, name + ": members", n=int(n.sum()))
    starts = host_ints(starts, name + ": starts", n=int(c.sum()) + b)
    for i, (m0, s0) in enumerate(zip(exclusive_offsets(n), exclusive_offsets(c + 1))):
        st, mem = starts[s0:s0 + c[i] + 1], members[m0:m0 + n[i]]
        if st[0] != 0 or st[-1] != n[i] or (np.diff(st) <= 0).any():
            raise ValueError("%s: recording %d: starts must ascend from 0 to its %d rows" % (name, i, int(n[i])))
        inner = np.ones(mem.size, bool)
        inner[st[:-1]] = False      # (the first member of a cluster need not be above the last of the cluster before)
        if not np.array_equal(np.sort(mem), np.arange(n[i])) or (np.diff(mem)[inner[1:]] <= 0).any() or (np.diff(mem[st[:-1]]) <= 0).any():
            raise ValueError("%s: recording %d: members must hold every row once, clusters ascending by their smallest member, a cluster's "
                             "members ascending" % (name, i))
    dev = scores.device
    seed = torch.empty(int((c * c).sum()), dtype=torch.float32, device=dev)
    sizes = torch.empty(int(c.sum()), dtype=torch.int32, device=dev)
    status = torch.empty(b, dtype=torch.int32, device=dev)
    ws_bytes = ahc_cluster_sums_workspace_bytes(n, c)
    ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=dev)
    off_d, n_d, ld_d, c_d = upload(mat_offsets, np.int64, dev), upload(n, np.int32, dev), upload(ld, np.int32, dev), upload(c, np.int32, dev)
    mem_d, st_d = upload(members, np.int32, dev), upload(starts, np.int32, dev)
    _lib.call("xv_ahc_cluster_sums", _s(), _p(scores), C.c_int64(scores.numel()), _p(off_d), _p(n_d), _p(ld_d), _p(c_d),
              _p(mem_d), _p(st_d), b, int(n.max()), int(c.max()), C.c_int64(int(n.sum())), C.c_int64(int(c.sum())),
              C.c_int64(int((c * c).sum())), C.c_int64(int((n * c).sum())), _p(seed), _p(sizes), _p(status), _p(ws), C.c_size_t(ws_bytes))
    if int(status.min()) != 0:
        raise RuntimeError("%s: xv_ahc_cluster_sums skipped recording %d" % (name, int(torch.argmin(status))))
    return seed, sizes


def ahc_subsets(n, first_pass_max_points):
    """The contiguous subsets of the first pass for a recording of n rows: ceil(n / first_pass_max_points) of them, ceil(n / that number)
    rows each, the last one shorter.  -> the boundaries, int64 [subsets + 1], from 0 to n."""
    n, cap = int(n), int(first_pass_max_points)
    subsets = -(-n // cap)
    size = -(-n // subsets)
    return np.minimum(np.arange(subsets + 1, dtype=np.int64) * size, n)


class TwoPassRefusal(ValueError):      # recording `recording` of an ahc_cluster_two_pass call is refused for `what`: for a caller that knows it by name
    def __init__(self, name, recording, what):
        ValueError.__init__(self, "%s: recording %d: %s" % (name, recording, what))
        self.recording, self.what = recording, what


def ahc_cluster_two_pass(scores, mat_offsets, n, ld=None, threshold=0.0, targets=None, first_pass_max_points=AHC_MAX_N):
    """Two-pass clustering of recordings of up to 32768 rows (Kaldi's AgglomerativeClusterer::ClusterTwoPass, recalled and restated - not
    compared with a Kaldi run, max_spk_fraction left out; tests/ahc2_ref.py restates this driver).  scores, mat_offsets, n, ld as for
    ahc_cluster.  targets None: every recording merges while the best average score is >= threshold; else targets[i] >= 1 clusters for
    every recording (a call has one stop rule).  A recording of more than first_pass_max_points (2 .. 2048) rows is cut into ahc_subsets;
    one ahc_cluster_from call clusters every subset of every recording down to min(its rows, 10 x max(target, 1)) clusters (or until the
    threshold stops it); ahc_cluster_sums adds up the scores between the surviving clusters, and one seeded ahc_cluster_from call merges
    them down to the target (threshold -inf) or the threshold (floor 1).  A row's label is the second-pass label of its first-pass
    cluster; final clusters are numbered by their smallest members.  A shorter recording is one subset that the first pass clusters to the
    end; its second pass merges nothing.  The first pass's labels come back to the host between the passes (one synchronisation).
    -> (labels int32 [sum n] on the device, first, second, subsets): first / second = (merges, merge_values, n_merges) of the two
    ahc_cluster_from calls - the first per subset in order, in the subset's row numbers; the second per recording, in first-pass cluster
    numbers -, subsets = [ahc_subsets(n[i])] per recording."""
    name = "ahc_cluster_two_pass"
    n, ld, mat_offsets = recordings(name, scores, mat_offsets, n, ld, AHC_MAX_POINTS)
    b, cap = n.size, int(first_pass_max_points)
    if not 2 <= cap <= AHC_MAX_N:
        raise ValueError("%s: first_pass_max_points must lie in 2 .. %d (got %d)" % (name, AHC_MAX_N, cap))
    if targets is None:
        targets = np.zeros(b, np.int64)
    else:
        targets = host_ints(targets, name + ": targets", n=b, dtype=np.int64)
        if (targets < 1).any() or (targets > n).any():
            i = int(np.argmax((targets < 1) | (targets > n)))
            raise ValueError("%s: recording %d: target %d outside 1 .. %d (None: the threshold, for every recording)" % (name, i, int(targets[i]), int(n[i])))
        threshold = float("-inf")
    ends = np.maximum(targets, 1)      # where a recording's merging may end at the latest
    subsets = [ahc_subsets(r, cap) for r in n]
    sub_off, sub_n, sub_ld, sub_floor = [], [], [], []
    for i, cuts in enumerate(subsets):
        rows = np.diff(cuts)
        sub_off.append(mat_offsets[i] + cuts[:-1] * (ld[i] + 1))
        sub_n.append(rows)
        sub_ld.append(np.full(rows.size, ld[i]))
        sub_floor.append(np.minimum(rows, 10 * ends[i]) if rows.size > 1 else ends[i:i + 1])
    sub_n = np.concatenate(sub_n)
    labels1, merges1, values1, n_merges1 = ahc_cluster_from(scores, np.concatenate(sub_off), sub_n, np.concatenate(sub_ld), floors=np.concatenate(sub_floor),
                                                            threshold=threshold)
    local = labels1.cpu().numpy().astype(np.int64)
    if int(n_merges1.min()) < 0:
        raise RuntimeError("%s: xv_ahc_cluster_from skipped subset %d" % (name, int(torch.argmin(n_merges1))))
    # a recording's first-pass clusters, numbered through its subsets: ascending by smallest member, since the subsets are contiguous
    clusters, c, at = np.empty(int(n.sum()), np.int64), np.zeros(b, np.int64), 0
    for i, cuts in enumerate(subsets):
        for rows in np.diff(cuts):
            clusters[at:at + rows] = c[i] + local[at:at + rows]
            c[i] += local[at:at + rows].max() + 1
            at += rows
        if c[i] > AHC_MAX_N:
            raise TwoPassRefusal(name, i, "the first pass leaves %d clusters, the second pass takes %d (lower the threshold or first_pass_max_points)"
                                 % (int(c[i]), AHC_MAX_N))
    members, starts, _ = ahc_member_lists(clusters, n)
    seed, _ = ahc_cluster_sums(scores, mat_offsets, n, ld, members, starts, c)
    sizes = np.concatenate([np.bincount(part) for part in np.split(clusters, bounds(n)[1:-1])])
    floors2 = np.where(n > cap, ends, c)      # (a short recording is done)
    labels2, merges2, values2, n_merges2 = ahc_cluster_from(None, None, c, floors=floors2, threshold=threshold, seed=seed, sizes=sizes)
    if int(n_merges2.min()) < 0:
        raise RuntimeError("%s: xv_ahc_cluster_from skipped recording %d in the second pass" % (name, int(torch.argmin(n_merges2))))
    index = upload(clusters + np.repeat(exclusive_offsets(c), n), np.int64, scores.device)
    return labels2[index], (merges1, values1, n_merges1), (merges2, values2, n_merges2), subsets


def ahc_cut(merges, merge_values, n_merges, n, thresholds, min_clusters=None, max_clusters=None):
    """The labels of b recordings at many cuts of one merge log, in one launch (xv_ahc_cut; include/xvector_hip.h states the rule,
    tests/diar_eval_ref.py restates it).  merges, merge_values, n_merges: ahc_cluster's outputs for recordings of n[i] rows, as it leaves
    them on the device - of a run with every target 1 for the labels of any threshold.  thresholds: HOST floats [cuts]; cut k applies the
    leading log entries whose value is >= thresholds[k] (float32), up to the first that fails, but leaves at least min_clusters[k] (None:
    1) and at most max_clusters[k] (None: no limit) clusters.  n, thresholds, min_clusters, max_clusters are checked here before the
    upload.  -> (labels int32 [cuts, sum n], clusters int32 [cuts, b]), device tensors; with the defaults cut k's labels are those of
    ahc_cluster(threshold=thresholds[k]), with min_clusters = max_clusters = t those of ahc_cluster(targets=t).  A recording whose
    n_merges is negative gets clusters -1."""
    name = "ahc_cut"
    n = host_ints(n, name + ": n", min_size=1, dtype=np.int64)
    if n.min() < 1 or n.max() > AHC_MAX_N:
        i = int(np.argmax((n < 1) | (n > AHC_MAX_N)))
        raise ValueError("%s: recording %d has %d rows, 1 .. %d are taken" % (name, i, int(n[i]), AHC_MAX_N))
    b, total = n.size, int(n.sum())
    thresholds = np.asarray(thresholds, dtype=np.float32)
    if thresholds.ndim != 1 or thresholds.size == 0:
        raise ValueError("%s: thresholds must be a non-empty 1-D array (cuts <= 0)" % name)
    if np.isnan(thresholds).any():
        raise ValueError("%s: threshold %d is NaN" % (name, int(np.argmax(np.isnan(thresholds)))))
    cuts = thresholds.size
    lo = np.ones(cuts, np.int32) if min_clusters is None else host_ints(min_clusters, name + ": min_clusters", n=cuts)
    hi = np.full(cuts, AHC_MAX_N, np.int32) if max_clusters is None else host_ints(max_clusters, name + ": max_clusters", n=cuts)
    if (lo < 1).any() or (hi < lo).any():
        k = int(np.argmax((lo < 1) | (hi < lo)))
        raise ValueError("%s: cut %d: min_clusters %d and max_clusters %d must satisfy 1 <= min_clusters <= max_clusters" % (name, k, int(lo[k]), int(hi[k])))
    for t, dtype, floats, what in ((merges, torch.int32, 2 * (total - b), "merges"), (merge_values, torch.float32, total - b, "merge_values"), (n_merges, torch.int32, b, "n_merges")):
        if t.dtype != dtype or not t.is_contiguous() or t.numel() != floats:
            raise ValueError("%s: %s must be a contiguous %s tensor of %d values (ahc_cluster's output for these recordings)" % (name, what, str(dtype).replace("torch.", ""), floats))
    dev = n_merges.device
    labels = torch.empty((cuts, total), dtype=torch.int32, device=dev)
    clusters = torch.empty((cuts, b), dtype=torch.int32, device=dev)
    n_d, t_d, lo_d, hi_d = upload(n, np.int32, dev), upload(thresholds, np.float32, dev), upload(lo, np.int32, dev), upload(hi, np.int32, dev)
    _lib.call("xv_ahc_cut", _s(), _p(merges), _p(merge_values), _p(n_merges), _p(n_d), b, int(n.max()), C.c_int64(total), _p(t_d), _p(lo_d), _p(hi_d), cuts,
              _p(labels), _p(clusters))
    return labels, clusters


# The reference of the recordings of diar_confusion calls, checked and on the device: ref_mask int32 (the bits of a uint32), scored uint8,
# frame_window int32 [sum frames]; frame_offsets, win_offsets int64 [b + 1] and speakers int32 [b] there, and frames, n, speakers on the host
DiarFrames = collections.namedtuple("DiarFrames", "ref_mask scored frame_window frame_offsets win_offsets speakers_d frames n speakers")


def diar_frames(ref_mask, scored, frame_window, frames, n, speakers, device):
    """The reference side of diar_confusion, uploaded once for every call (every batch of cuts) that scores against it.  HOST arrays, the
    recordings back to back: ref_mask uint32 [sum frames] (bit s: reference speaker s talks), scored [sum frames] (0: not scored),
    frame_window int32 [sum frames] (the window of its recording that owns the frame, -1: none); frames, n, speakers [b]: the frames,
    windows and reference speakers (1 .. 32) of each recording.  Checked here - the kernel trusts them.  -> DiarFrames."""
    name = "diar_frames"
    frames = host_ints(frames, name + ": frames", min_size=1, dtype=np.int64)
    b = frames.size
    n = host_ints(n, name + ": n", n=b, dtype=np.int64)
    speakers = host_ints(speakers, name + ": speakers", n=b, dtype=np.int64)
    if frames.min() < 0 or n.min() < 1:
        raise ValueError("%s: recording %d has %d frames and %d windows" % (name, int(np.argmax((frames < 0) | (n < 1))), int(frames.min()), int(n.min())))
    if speakers.min() < 1 or speakers.max() > DIAR_MAX_SPEAKERS:
        i = int(np.argmax((speakers < 1) | (speakers > DIAR_MAX_SPEAKERS)))
        raise ValueError("%s: recording %d has %d reference speakers, 1 .. %d are taken" % (name, i, int(speakers[i]), DIAR_MAX_SPEAKERS))
    total = int(frames.sum())
    ref_mask, scored, frame_window = np.asarray(ref_mask), np.asarray(scored), np.asarray(frame_window)
    if ref_mask.dtype != np.uint32 or ref_mask.shape != (total,):
        raise ValueError("%s: ref_mask must be a uint32 array of %d frames" % (name, total))
    if scored.shape != (total,) or scored.dtype.kind not in "biu":
        raise ValueError("%s: scored must be a boolean or integer array of %d frames" % (name, total))
    frame_window = host_ints(frame_window, name + ": frame_window", n=total)
    at = bounds(frames)
    for i in range(b):
        own, mask = frame_window[at[i]:at[i + 1]], ref_mask[at[i]:at[i + 1]]
        if own.size and (own.min() < -1 or own.max() >= n[i]):
            raise IndexError("%s: recording %d: frame_window holds a value outside -1 .. %d" % (name, i, int(n[i]) - 1))
        if mask.size and speakers[i] < 32 and int(mask.max()) >> int(speakers[i]):
            raise ValueError("%s: recording %d: ref_mask has a bit at or above its %d speakers" % (name, i, int(speakers[i])))
    return DiarFrames(upload(ref_mask.view(np.int32), np.int32, device), upload(scored != 0, np.uint8, device), upload(frame_window, np.int32, device),
                      upload(at, np.int64, device), upload(bounds(n), np.int64, device), upload(speakers, np.int32, device), frames, n, speakers)


def diar_confusion(reference, labels, clusters):
    """Diarization error counts of b recordings at many cuts in one launch (xv_diar_confusion; include/xvector_hip.h states the
    arithmetic, tests/diar_eval_ref.py restates it).  reference: diar_frames' result.  labels: int32 [cuts, sum n] on the device, a window's
    cluster in 0 .. clusters - 1 (ahc_cut's labels, or VBx's); clusters: int [cuts, b], the clusters of each (cut, recording) - a device
    tensor (ahc_cut's: it comes to the host here, one synchronisation) or a host array.
    -> (totals int64 [cuts, b, 3] = (scored speaker time, miss, false alarm) in frames; overlap int32 1-D, the frames reference speaker s
    shares with cluster h, the block of (cut k, recording i) packed [speakers[i], clusters[k, i]] at out_offsets[k, i]; out_offsets HOST
    int64 [cuts, b]; status int32 [cuts, b]: 0 counted, 1 not counted - more than 256 clusters -, -1 not counted - clusters below 1 or
    entries out of range), the tensors on the device.  All integers: exact, and the same bytes every time."""
    name = "diar_confusion"
    b, total_n = reference.n.size, int(reference.n.sum())
    if labels.dtype != torch.int32 or labels.dim() != 2 or labels.shape[1] != total_n or labels.shape[0] < 1 or not labels.is_contiguous():
        raise ValueError("%s: labels must be a contiguous int32 [cuts, %d] tensor" % (name, total_n))
    cuts, dev = labels.shape[0], labels.device
    host = clusters.cpu().numpy() if isinstance(clusters, torch.Tensor) else np.asarray(clusters)
    if host.shape != (cuts, b) or host.dtype.kind not in "iu":
        raise ValueError("%s: clusters must be an integer [%d, %d] array" % (name, cuts, b))
    host = host.astype(np.int64)
    sizes = np.where((host >= 1) & (host <= DIAR_MAX_CLUSTERS), host * reference.speakers[None, :], 0).reshape(-1)      # (a block that is not counted holds nothing)
    out_offsets = exclusive_offsets(sizes).reshape(cuts, b)
    overlap_ints = int(sizes.sum())
    totals = torch.empty((cuts, b, 3), dtype=torch.int64, device=dev)
    overlap = torch.empty(max(overlap_ints, 1), dtype=torch.int32, device=dev)
    status = torch.empty((cuts, b), dtype=torch.int32, device=dev)
    c_d, o_d = upload(host.reshape(-1), np.int32, dev), upload(out_offsets.reshape(-1), np.int64, dev)
    _lib.call("xv_diar_confusion", _s(), _p(reference.ref_mask), _p(reference.scored), _p(reference.frame_window), _p(reference.frame_offsets),
              _p(reference.win_offsets), _p(reference.speakers_d), b, C.c_int64(int(reference.frames.sum())), C.c_int64(total_n), _p(labels), _p(c_d), _p(o_d), cuts,
              C.c_int64(overlap_ints), _p(totals), _p(overlap), _p(status))
    return totals, overlap[:overlap_ints], out_offsets, status


def vbx_workspace_bytes(t, s, d):
    """Bytes of scratch xv_vbx needs for recordings of t[i] rows and s[i] speakers (host integer arrays of one length) in d dimensions."""
    t, s = np.asarray(t, dtype=np.int64), np.asarray(s, dtype=np.int64)
    return int(_lib.load().xv_vbx_workspace_bytes(C.c_int64(int(t.sum())), C.c_int64(int((t * s).sum())), C.c_int64(int(s.sum())), int(d)))


def vbx(x, x_offsets, t, d, phi, gamma, pi, s, ld=None, loop_prob=0.99, fa=0.3, fb=17.0, max_iters=20, epsilon=1e-4):
    """VB-HMM clustering (VBx) of b recordings in one call (xv_vbx; include/xvector_hip.h states the arithmetic, tests/vbx_ref.py restates
    it).  x: a contiguous 1-D float32 device buffer; recording i's rows [t[i], ld[i]] (ld None: d) start at float x_offsets[i]: vectors in
    the PLDA space with within-class covariance I and between-class covariance diag(phi) (BackendScorer.plda_space).  phi: float32 [d]
    on the device.  gamma: the initial responsibilities, recording i's [t[i], s[i]] back to back in one 1-D float32 device tensor; pi: the
    initial priors, recording i's [s[i]] back to back.  x_offsets, t, ld, s: HOST integer arrays, checked here before the upload - the
    kernel trusts them.  epsilon: the smallest gain of the ELBO that keeps iterating (-inf: always max_iters).
    -> (gamma, pi, elbo float64 [b, max_iters] - NaN behind the iterations run -, n_iters int32 [b], labels int32 [sum t]), device tensors
    laid out as the inputs; x, phi and the initial gamma and pi are not modified."""
    d, max_iters = int(d), int(max_iters)
    if not 1 <= d <= VBX_MAX_DIM:
        raise ValueError("vbx: d must lie in 1 .. %d (got %d)" % (VBX_MAX_DIM, d))
    if not 1 <= max_iters <= VBX_MAX_ITERS:
        raise ValueError("vbx: max_iters must lie in 1 .. %d (got %d)" % (VBX_MAX_ITERS, max_iters))
    loop32 = float(np.float32(loop_prob))
    if not 0.0 < loop32 < 1.0:
        raise ValueError("vbx: loop_prob must lie strictly between 0 and 1 as a float32 (got %r)" % (loop_prob,))
    if not (float(np.float32(fa)) > 0.0 and float(np.float32(fb)) > 0.0 and np.isfinite(np.float32(fa)) and np.isfinite(np.float32(fb))):
        raise ValueError("vbx: fa and fb must be positive (got %r, %r)" % (fa, fb))
    if np.isnan(epsilon):
        raise ValueError("vbx: epsilon is not a number")
    t, ld, x_offsets = recordings("vbx", x, x_offsets, t, ld, VBX_MAX_ROWS, letter="t", d=d)
    b = t.size
    s = host_ints(s, "vbx: s", n=b, dtype=np.int64)
    if s.min() < 1:
        raise ValueError("vbx: recording %d has no speaker (s = %d)" % (int(np.argmax(s < 1)), int(s.min())))
    if s.max() > VBX_MAX_SPEAKERS:
        raise ValueError("vbx: recording %d has %d speakers, the cap is %d" % (int(np.argmax(s > VBX_MAX_SPEAKERS)), int(s.max()), VBX_MAX_SPEAKERS))
    total_t, total_ts, total_s = int(t.sum()), int((t * s).sum()), int(s.sum())
    f32_values(phi, d, "vbx: phi")
    f32_values(gamma, total_ts, "vbx: gamma (sum of t * s)")
    f32_values(pi, total_s, "vbx: pi (sum of s)")
    dev = x.device
    gamma_out, pi_out = torch.empty_like(gamma), torch.empty_like(pi)
    elbo = torch.full((b, max_iters), float("nan"), dtype=torch.float64, device=dev)
    n_iters = torch.empty(b, dtype=torch.int32, device=dev)
    labels = torch.empty(total_t, dtype=torch.int32, device=dev)
    ws_bytes = vbx_workspace_bytes(t, s, d)
    ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=dev)
    off_d, t_d, ld_d, s_d = upload(x_offsets, np.int64, dev), upload(t, np.int32, dev), upload(ld, np.int32, dev), upload(s, np.int32, dev)
    _lib.call("xv_vbx", _s(), _p(x), C.c_int64(x.numel()), _p(off_d), _p(t_d), _p(ld_d), _p(s_d), b, d, int(t.max()), int(s.max()), C.c_int64(total_t),
              C.c_int64(total_ts), C.c_int64(total_s), _p(phi), _p(gamma), _p(pi), C.c_float(loop32), C.c_float(float(fa)), C.c_float(float(fb)),
              max_iters, C.c_double(float(epsilon)), _p(gamma_out), _p(pi_out), _p(elbo), _p(n_iters), _p(labels), _p(ws), C.c_size_t(ws_bytes))
    return gamma_out, pi_out, elbo, n_iters, labels


def backend_pca_plda_workspace_bytes(b, d):
    """Bytes of scratch xv_backend_pca_plda needs for b recordings in d dimensions."""
    return int(_lib.load().xv_backend_pca_plda_workspace_bytes(int(b), int(d)))


def backend_pca_plda(x, x_offsets, n, d, w, b, mu, target, ld=None):
    """The per-recording PCA of ivector-plda-scoring-dense --target-energy for the recordings of one call (xv_backend_pca_plda;
    include/xvector_hip.h states the arithmetic, tests/pca_plda_ref.py restates it).  x: a contiguous 1-D float32 device buffer; recording
    i's rows [n[i], ld[i]] (ld None: d) start at float x_offsets[i]: centred, LDA-transformed, unit-length vectors.  w, b: float64 [d, d]
    device tensors, the within- and between-class covariances of the PLDA model (misc.backend.plda_covariances); mu: float64 [d], its
    mean.  target: the share of the energy to keep, in (0, 1].  x_offsets, n, ld: HOST integer arrays, checked here before the upload - the
    kernel trusts them.
    -> dict of device tensors, d4 = d rounded up to 4: p int32 [recordings] (0: no PCA for this recording, use the global model; -2 / -3: the
    eigensolver reached its sweep cap / the projected within-class covariance is not positive definite), a float32 [recordings, d4, d4] (the
    first p rows and d columns hold the map, the rest zero), offset, psi, g float32 [recordings, d4], coef float32 [recordings, 2, d4],
    k0 float32 [recordings], s, psi64 float64 [recordings, d], sweeps int32 [recordings, 2].  What the kernel does not write - everything
    but p (and s) of a recording with p <= 0, psi64 behind p - stays NaN (sweeps: -1)."""
    d, target = int(d), float(target)
    if not 1 <= d <= PCA_MAX_DIM:
        raise ValueError("backend_pca_plda: d must lie in 1 .. %d (got %d)" % (PCA_MAX_DIM, d))
    if not 0.0 < target <= 1.0:
        raise ValueError("backend_pca_plda: target must lie in (0, 1] (got %r)" % (target,))
    n, ld, x_offsets = recordings("backend_pca_plda", x, x_offsets, n, ld, PCA_MAX_ROWS, d=d)
    count = n.size
    for t, shape, name in ((w, (d, d), "w"), (b, (d, d), "b"), (mu, (d,), "mu")):
        if t.dtype != torch.float64 or tuple(t.shape) != shape or not t.is_contiguous() or t.device != x.device:
            raise ValueError("backend_pca_plda: %s must be a contiguous float64 %s tensor on the rows' device" % (name, list(shape)))
    dev, d4 = x.device, pitch4(d)
    nan32 = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device=dev)
    out = dict(p=torch.empty(count, dtype=torch.int32, device=dev), a=nan32(count, d4, d4), offset=nan32(count, d4), psi=nan32(count, d4),
               coef=nan32(count, 2, d4), g=nan32(count, d4), k0=nan32(count),
               s=torch.full((count, d), float("nan"), dtype=torch.float64, device=dev),
               psi64=torch.full((count, d), float("nan"), dtype=torch.float64, device=dev),
               sweeps=torch.full((count, 2), -1, dtype=torch.int32, device=dev))
    ws_bytes = backend_pca_plda_workspace_bytes(count, d)
    ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=dev)
    off_d, n_d, ld_d = upload(x_offsets, np.int64, dev), upload(n, np.int32, dev), upload(ld, np.int32, dev)
    _lib.call("xv_backend_pca_plda", _s(), _p(x), C.c_int64(x.numel()), _p(off_d), _p(n_d), _p(ld_d), count, d, int(n.max()), C.c_double(target),
              _p(w), _p(b), _p(mu), _p(out["p"]), _p(out["a"]), _p(out["offset"]), _p(out["psi"]), _p(out["coef"]), _p(out["g"]), _p(out["k0"]),
              _p(out["s"]), _p(out["psi64"]), _p(out["sweeps"]), _p(ws), C.c_size_t(ws_bytes))
    return out
