"""Labels at many cuts of one merge log on a real MI355X: xv_ahc_cut through ops.ahc_cut.

A threshold changes the clusterer's stop rule and nothing else, so the check needs no tolerance: the cut of the log of a run down to one
cluster must EQUAL, label for label, what ops.ahc_cluster gives when it is run with that threshold (or that target) - at every size at
which either kernel takes another path (one row, one wave, a second column per thread, the cap), on random scores and on integer-valued
ones whose logs are full of ties, and at thresholds that are logged values themselves.  The hand-written logs of
tests/test_diar_eval_ref.py go through the kernel against the restatement."""
import numpy as np
import pytest

from tests import diar_eval_ref as R
from tests.test_diar_eval_ref import CUTS, LOGS

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SIZES = (1, 2, 3, 64, 65, 255, 256, 257)
INF = float("inf")


def _ops():
    import torch
    from tf_kaldi_speaker_amd import ops
    return torch, ops


_RUNS = {}


def _run(kind, sizes):
    """Scores of `kind` for recordings of `sizes` rows in one packed buffer, and the log of ops.ahc_cluster down to one cluster; built once."""
    if (kind, sizes) not in _RUNS:
        torch, ops = _ops()
        rs = np.random.RandomState(len(sizes) + (7 if kind == "ties" else 0))
        n = np.asarray(sizes, np.int64)
        mats = [rs.randint(-2, 3, (k, k)).astype(np.float32) if kind == "ties" else rs.randn(k, k).astype(np.float32) for k in sizes]
        buf = torch.from_numpy(np.concatenate([m.ravel() for m in mats])).to(DEV)
        off = np.concatenate([[0], np.cumsum(n * n)])[:-1]
        log = ops.ahc_cluster(buf, off, n, targets=np.ones(n.size, np.int64))
        assert log[3].cpu().numpy().tolist() == (n - 1).tolist()
        _RUNS[kind, sizes] = (buf, off, n, log)
    return _RUNS[kind, sizes]


def _thresholds(log, n):
    """-inf, +inf, 0, and from every recording's log some logged values themselves, and the float32 above and below one of them."""
    values, at = log[2].cpu().numpy(), np.concatenate([[0], np.cumsum(n - 1)])
    out = [-INF, INF, 0.0]
    for i in range(n.size):
        own = values[at[i]:at[i + 1]]
        if own.size:
            picked = own[[0, own.size // 2, own.size - 1]]
            out += [float(v) for v in picked] + [float(np.nextafter(picked[1], np.float32(9))), float(np.nextafter(picked[1], np.float32(-9)))]
    return sorted(set(out))


@pytest.mark.parametrize("kind,sizes", [("random", SIZES), ("ties", SIZES), ("random", (2048,)), ("ties", (2048,))])
def test_cuts_equal_the_clusterer_run_with_each_threshold(kind, sizes):
    torch, ops = _ops()
    buf, off, n, log = _run(kind, sizes)
    thresholds = _thresholds(log, n)
    labels, clusters = ops.ahc_cut(log[1], log[2], log[3], n, thresholds)
    assert labels.shape == (len(thresholds), int(n.sum())) and clusters.shape == (len(thresholds), n.size) and labels.dtype == clusters.dtype == torch.int32
    at = np.concatenate([[0], np.cumsum(n)])
    counts = clusters.cpu().numpy()
    for k, threshold in enumerate(thresholds):
        want = ops.ahc_cluster(buf, off, n, threshold=threshold)[0]
        assert torch.equal(labels[k], want), (kind, threshold)
        assert counts[k].tolist() == [int(want[lo:hi].max()) + 1 for lo, hi in zip(at[:-1], at[1:])]
    if kind == "ties":
        assert np.unique(log[2].cpu().numpy()).size < (n.sum() - n.size) // 2      # (the log does repeat its values)
    # the same bytes from a second call
    again = ops.ahc_cut(log[1], log[2], log[3], n, thresholds)
    assert torch.equal(again[0], labels) and torch.equal(again[1], clusters)


@pytest.mark.parametrize("kind", ["random", "ties"])
def test_min_and_max_clusters_give_the_clusterer_run_to_a_target(kind):
    torch, ops = _ops()
    buf, off, n, log = _run(kind, SIZES)
    targets = [1, 2, 3, 64, 200, 257]
    # whatever the threshold says: +inf would merge nothing, -inf everything
    for threshold in (INF, -INF):
        labels, clusters = ops.ahc_cut(log[1], log[2], log[3], n, [threshold] * len(targets), min_clusters=targets, max_clusters=targets)
        for k, t in enumerate(targets):
            want = ops.ahc_cluster(buf, off, n, targets=np.minimum(t, n))[0]
            assert torch.equal(labels[k], want), (kind, threshold, t)
            assert clusters[k].cpu().numpy().tolist() == np.minimum(t, n).tolist()
    # the two clamps around a threshold: at least 2 and at most 5 clusters
    mid = float(np.median(log[2].cpu().numpy()))
    labels, clusters = ops.ahc_cut(log[1], log[2], log[3], n, [-INF, mid, INF], min_clusters=[2, 2, 2], max_clusters=[5, 5, 5])
    by_threshold = ops.ahc_cluster(buf, off, n, threshold=mid)[0].cpu().numpy()
    at = np.concatenate([[0], np.cumsum(n)])
    free = np.asarray([int(by_threshold[lo:hi].max()) + 1 for lo, hi in zip(at[:-1], at[1:])])
    assert clusters.cpu().numpy().tolist() == [np.minimum(2, n).tolist(), np.minimum(np.clip(free, 2, 5), n).tolist(), np.minimum(5, n).tolist()]


def test_hand_written_logs_match_the_restatement_and_a_bad_recording_is_skipped():
    torch, ops = _ops()
    names = list(LOGS)
    n = np.asarray([LOGS[k][0] for k in names], np.int64)
    slots = int((n - 1).sum())
    merges, values, n_merges = np.full((slots, 2), -7, np.int32), np.full(slots, np.nan, np.float32), np.zeros(n.size, np.int32)
    for i, (k, lo) in enumerate(zip(names, np.concatenate([[0], np.cumsum(n - 1)]))):
        m = len(LOGS[k][1])
        merges[lo:lo + m], values[lo:lo + m], n_merges[i] = np.asarray(LOGS[k][1], np.int32).reshape(m, 2), LOGS[k][2], m
    up = lambda a: torch.from_numpy(a).to(DEV)
    thresholds = [c[0] for c in CUTS]
    lo_hi = dict(min_clusters=[c[1] for c in CUTS], max_clusters=[2048 if c[2] is None else c[2] for c in CUTS])
    labels, clusters = (t.cpu().numpy() for t in ops.ahc_cut(up(merges), up(values), up(n_merges), n, thresholds, **lo_hi))
    at = np.concatenate([[0], np.cumsum(n)])
    for k, c in enumerate(CUTS):
        for i, name in enumerate(names):
            want, count = R.cut(LOGS[name][1], LOGS[name][2], LOGS[name][0], *c)
            assert labels[k, at[i]:at[i + 1]].tolist() == want.tolist() and clusters[k, i] == count, (name, c)
    # n_merges = -1 (a recording the clusterer skipped): clusters = -1 in every cut, the others as before; so is a log that leads outside
    n_merges[1] = -1
    merges[0] = (3, 9)      # recording 0 ("chain", 5 rows): an entry without a < b < n
    _, bad = ops.ahc_cut(up(merges), up(values), up(n_merges), n, thresholds, **lo_hi)
    bad = bad.cpu().numpy()
    assert (bad[:, 1] == -1).all() and np.array_equal(bad[:, 2:], clusters[:, 2:])
    assert [bad[k, 0] for k, c in enumerate(CUTS)] == [-1 if clusters[k, 0] < 5 else 5 for k in range(len(CUTS))]      # (a cut that applies no merge reads no entry)


def test_refusals_by_name():
    torch, ops = _ops()
    _, _, n, log = _run("random", SIZES)
    with pytest.raises(ValueError, match="^ahc_cut: threshold 1 is NaN$"):
        ops.ahc_cut(log[1], log[2], log[3], n, [0.0, float("nan")])
    with pytest.raises(ValueError, match="^ahc_cut: thresholds must be a non-empty 1-D array \\(cuts <= 0\\)$"):
        ops.ahc_cut(log[1], log[2], log[3], n, [])
    with pytest.raises(ValueError, match="^ahc_cut: cut 1: min_clusters 0 and max_clusters 2048 must satisfy 1 <= min_clusters <= max_clusters$"):
        ops.ahc_cut(log[1], log[2], log[3], n, [0.0, 0.0], min_clusters=[1, 0])
    with pytest.raises(ValueError, match="^ahc_cut: cut 0: min_clusters 3 and max_clusters 2 must satisfy"):
        ops.ahc_cut(log[1], log[2], log[3], n, [0.0], min_clusters=[3], max_clusters=[2])
    with pytest.raises(ValueError, match="^ahc_cut: recording 2 has 2049 rows, 1 .. 2048 are taken$"):
        ops.ahc_cut(log[1], log[2], log[3], [1, 2, 2049], [0.0])
    with pytest.raises(ValueError, match="^ahc_cut: merges must be a contiguous int32 tensor of %d values" % (2 * int(n.sum() - n.size + 1))):
        ops.ahc_cut(log[1], log[2], log[3], np.concatenate([n[:-1], n[-1:] + 1]), [0.0])
    from tf_kaldi_speaker_amd import _lib
    import ctypes as C
    lib = _lib.load()
    for args, what in (((0, 4, 0, 1), "ahc_cut: no recording in the call (b=0)"), ((1, 2049, 2049, 1), "ahc_cut: a recording of 2049 rows exceeds the cap of 2048"),
                       ((2, 4, 9, 1), "ahc_cut: total_n does not fit b recordings of at most 4 rows"), ((1, 4, 4, 0), "ahc_cut: 1 .. 65535 cuts in a call (cuts=0)")):
        b, max_n, total, cuts = args
        rc = lib.xv_ahc_cut(None, None, None, None, None, b, max_n, C.c_int64(total), None, None, None, cuts, None, None)
        assert rc == 2 and lib.xv_last_error().decode() == what
