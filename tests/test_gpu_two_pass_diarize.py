"""Two-pass clustering of long recordings on a real MI355X: ops.ahc_cluster_two_pass and Diarizer(first_pass_max_points=...) against the
restatement tests/ahc2_ref.py driven by the same GPU score matrix, the unchanged path of short recordings, the default setting at the
first size that takes the new path (2049 windows), the named refusals, and nnet/lib/diarize.py --first-pass-max-points end to end."""
import os

import numpy as np
import pytest

from tests import ahc2_ref as R2
from tests.test_ahc2_ref import _partition
from tests.test_gpu_ahc import DEV, _split

pytestmark = pytest.mark.gpu

DIM = 16


def _recording(seed, n, k, spread=0.04):
    """Windows of k well-separated speakers that recur all along the recording (tests/test_ahc2_ref.py's blobs, as embeddings)."""
    rs = np.random.RandomState(seed)
    while True:
        means = rs.randn(k, DIM)
        means /= np.linalg.norm(means, axis=1, keepdims=True)
        if k == 1 or (means @ means.T - np.eye(k)).max() < 0.6:
            break
    who = rs.randint(0, k, n)
    who[:k] = np.arange(k)
    return (means[who] + spread * rs.randn(n, DIM)).astype(np.float32), who


def _scorer():
    from tf_kaldi_speaker_amd.misc import scoring as S
    return S.CosineScorer(DEV)


THRESHOLD = 0.75      # between the two score populations of _long()'s recordings, which _long() asserts

_LONG = {}


def _long():
    """Three recordings of 70 - 150 windows: {name: (embeddings, speakers, the scorer's dense matrix on the host)}; built once."""
    if not _LONG:
        scorer = _scorer()
        for name, n, k in (("recA", 70, 3), ("recB", 97, 2), ("recC", 150, 4)):
            x, who = _recording(n, n, k)
            s = scorer.dense(scorer.prepare(x)).cpu().numpy()
            same = np.equal.outer(who, who)
            upper = np.triu(np.ones_like(same), 1)
            assert s[~same & upper].max() < 0.7 < 0.85 < s[same & upper].min()      # the condition on the inputs (tests/test_ahc2_ref.py)
            _LONG[name] = (x, who, s)
    return _LONG


def test_the_op_is_the_restatement_driven_by_the_same_scores():
    import torch
    from tf_kaldi_speaker_amd import ops
    recos = _long()
    mats = [s for _, _, s in recos.values()]
    n = np.asarray([m.shape[0] for m in mats], np.int64)
    ld = n + 2
    off = np.concatenate([[0], np.cumsum(n * ld)])[:-1]
    host = np.full(int((n * ld).sum()), np.nan, np.float32)
    for m, o, r, l in zip(mats, off, n, ld):
        host[o:o + r * l].reshape(r, l)[:, :r] = m
    buf = torch.from_numpy(host).to(DEV)
    for kw, targets in ((dict(threshold=THRESHOLD), None), (dict(), [3, 2, 4]), (dict(), [1, 5, 150])):
        labels, first, second, subsets = ops.ahc_cluster_two_pass(buf, off, n, ld, first_pass_max_points=32, targets=targets, **kw)
        labels = labels.cpu().numpy()
        # the two merge logs, cut per subset and per recording (a recording's second pass starts from what its subsets left)
        sub_n = np.concatenate([np.diff(b) for b in subsets]).astype(np.int32)
        first = _split((torch.zeros(int(sub_n.sum()), dtype=torch.int32),) + first, sub_n)
        left = [int(r) - len(f[1]) for r, f in zip(sub_n, first)]
        ends = np.cumsum([len(b) - 1 for b in subsets])
        c = np.asarray([sum(left[i:j]) for i, j in zip(np.concatenate([[0], ends[:-1]]), ends)], np.int32)
        second = _split((torch.zeros(int(c.sum()), dtype=torch.int32),) + second, c)
        at, sub = np.concatenate([[0], np.cumsum(n)]), 0
        for i, m in enumerate(mats):
            want = R2.two_pass(m, target=0 if targets is None else targets[i], first_pass_max_points=32, **kw)
            assert subsets[i].tolist() == want[3] == R2.subsets(int(n[i]), 32)
            assert labels[at[i]:at[i + 1]].tolist() == want[0].tolist()
            for (merges, vals) in want[1]:      # the first pass's log, subset by subset, bit for bit
                assert first[sub][1].tolist() == merges.tolist() and first[sub][2].view(np.int32).tolist() == vals.view(np.int32).tolist()
                sub += 1
            assert second[i][1].tolist() == want[2][0].tolist() and second[i][2].view(np.int32).tolist() == want[2][1].view(np.int32).tolist()
        if targets is None or targets == [3, 2, 4]:      # on these recordings that is the truth, and what one pass finds
            for i, (_, who, m) in enumerate(recos.values()):
                assert labels[at[i]:at[i + 1]].tolist() == _partition(who)


def test_diarizer_with_short_and_long_recordings_in_one_call():
    from tf_kaldi_speaker_amd.misc import diarization as D
    scorer = _scorer()
    recos = _long()
    short = {"s%d" % i: _recording(40 + i, n, k)[0] for i, (n, k) in enumerate(((32, 2), (9, 3), (1, 1), (31, 2)))}
    emb = {"s0": short["s0"], "recA": recos["recA"][0], "s1": short["s1"], "recC": recos["recC"][0], "s2": short["s2"], "recB": recos["recB"][0],
           "s3": short["s3"]}
    threshold = THRESHOLD
    num = {k: (int(recos[k][1].max()) + 1 if k in recos else 2) for k in emb}
    by_threshold = None
    for kw in (dict(threshold=threshold), dict(reco2num_spk=num)):
        got = D.Diarizer(scorer, first_pass_max_points=32, **kw).cluster(emb)
        by_threshold = by_threshold or got
        assert list(got) == list(emb)
        plain = D.Diarizer(scorer, **kw).cluster(short)      # without the option: today's path
        for k in short:
            assert got[k].dtype == plain[k].dtype and got[k].tolist() == plain[k].tolist()
        for k, (x, who, s) in recos.items():
            want = R2.two_pass(s, first_pass_max_points=32, **(dict(threshold=threshold) if "threshold" in kw else dict(target=num[k])))
            assert got[k].tolist() == want[0].tolist() == _partition(who)
    # one recording per batch: a workspace that holds the largest long recording alone gives the same labels; one byte less is refused
    diar = D.Diarizer(scorer, threshold=threshold, first_pass_max_points=32)
    need = diar._two_pass_bytes(150, 152, 0)
    scorer.workspace_bytes = need
    assert {k: v.tolist() for k, v in diar.cluster(emb).items()} == {k: v.tolist() for k, v in by_threshold.items()}
    scorer.workspace_bytes = need - 1
    with pytest.raises(ValueError, match="recording recC needs %d bytes of scores, the workspace holds %d" % (need, need - 1)):
        diar.cluster(emb)


def test_2049_windows_at_the_default_setting():
    """The smallest recording that takes the new path by default; the parent commit refuses it ("has 2049 windows, 1 .. 2048 are taken")."""
    from tf_kaldi_speaker_amd.misc import diarization as D
    x, who = _recording(2049, 2049, 5)
    scorer = _scorer()
    s = scorer.dense(scorer.prepare(x)).cpu().numpy()
    same = np.equal.outer(who, who)
    upper = np.triu(np.ones_like(same), 1)
    lo, hi = s[~same & upper].max(), s[same & upper].min()
    assert lo < hi      # the condition on the inputs: every same-speaker score above every other
    for kw in (dict(threshold=0.5 * (float(lo) + float(hi))), dict(reco2num_spk={"long": 5})):
        labels = D.Diarizer(scorer, **kw).cluster({"long": x})["long"]
        assert labels.shape == (2049,) and int(labels.max()) + 1 == 5
        assert labels.tolist() == _partition(who)


def test_refusals():
    import torch
    from tf_kaldi_speaker_amd import ops
    from tf_kaldi_speaker_amd.misc import backend as B
    from tf_kaldi_speaker_amd.misc import diarization as D
    scorer = _scorer()
    x, _ = _recording(1, 2049, 2)
    with pytest.raises(ValueError, match="first_pass_max_points must lie in 2 .. 2048"):
        D.Diarizer(scorer, threshold=0.5, first_pass_max_points=1)
    with pytest.raises(ValueError, match="first_pass_max_points must lie in 2 .. 2048"):
        D.Diarizer(scorer, threshold=0.5, first_pass_max_points=2049)
    # a back end in the plda mode, for the two options that keep their cap of 2048 windows
    rs = np.random.RandomState(3)
    spk = rs.randn(20, DIM)
    train = (np.repeat(spk, 6, axis=0) + 0.2 * rs.randn(120, DIM)).astype(np.float32)
    keys = ["u%03d" % i for i in range(120)]
    backend = B.Backend.train(train, keys, [("s%02d" % s, keys[6 * s:6 * s + 6]) for s in range(20)], lda_dim=8, device=DEV)
    plda = B.BackendScorer(backend, "plda", DEV)
    with pytest.raises(ValueError, match="recording long has 2049 windows: vbx= takes recordings of at most 2048 \\(xv_vbx keeps its cap"):
        D.Diarizer(plda, threshold=0.0, vbx=D.VbxOptions()).cluster({"ok": x[:50], "long": x})
    with pytest.raises(ValueError, match="recording long has 2049 windows: target_energy= takes recordings of at most 2048 \\(xv_backend_pca_plda"):
        D.Diarizer(plda, threshold=0.0, target_energy=0.9).cluster({"long": x})
    with pytest.raises(ValueError, match="recording long has 32769 windows, 1 .. 32768 are taken"):
        D.Diarizer(scorer, threshold=0.5).cluster({"long": np.zeros((32769, DIM), np.float32)})
    # a threshold no score reaches: the first pass merges nothing and leaves more clusters than the second pass takes
    with pytest.raises(ValueError, match="recording long: the first pass leaves 2049 clusters, the second pass takes 2048 \\(lower the threshold or "
                                         "first_pass_max_points\\)"):
        D.Diarizer(scorer, threshold=2.0).cluster({"ok": x[:50], "long": x})
    buf = torch.zeros(2049 * 2049, dtype=torch.float32, device=DEV)
    with pytest.raises(ValueError, match="the first pass leaves 2049 clusters"):
        ops.ahc_cluster_two_pass(buf, [0], [2049], threshold=1.0)
    with pytest.raises(ValueError, match="first_pass_max_points must lie in 2 .. 2048 \\(got 1\\)"):
        ops.ahc_cluster_two_pass(buf, [0], [64], first_pass_max_points=1)
    with pytest.raises(ValueError, match="first_pass_max_points must lie in 2 .. 2048 \\(got 4096\\)"):
        ops.ahc_cluster_two_pass(buf, [0], [64], first_pass_max_points=4096)
    with pytest.raises(ValueError, match="recording 0 has 32769 rows, the cap is 32768"):
        ops.ahc_cluster_two_pass(buf, [0], [32769])
    with pytest.raises(ValueError, match="target 0 outside 1 .. 64"):
        ops.ahc_cluster_two_pass(buf, [0, 0], [64, 64], targets=[2, 0])
    with pytest.raises(ValueError, match="the pitch 63 is below its 64 rows"):
        ops.ahc_cluster_two_pass(buf, [0], [64], [63])
    with pytest.raises(IndexError, match="a matrix lies outside"):
        ops.ahc_cluster_two_pass(buf, [2049 * 2049 - 100], [64])


def test_driver_with_first_pass_max_points(tmp_path):
    """nnet/lib/diarize.py --first-pass-max-points on a tiny archive: the RTTM is what the planner's windows, the written embeddings, the
    scorer's dense matrix and the restated two-pass driver give."""
    from tests.test_gpu_diarize import RTTM_LINE, _diarize, _model
    from tf_kaldi_speaker_amd.dataset import kaldi_io
    from tf_kaldi_speaker_amd.misc import diarization as D
    tmp = str(tmp_path)
    model = os.path.join(tmp, "exp")
    _model(model)
    rs = np.random.RandomState(23)
    frames = 3000
    tilt = np.where((np.arange(frames)[:, None] // 500) % 2 == 0, np.linspace(-2, 2, 30)[None, :], np.linspace(2, -2, 30)[None, :])
    with open(os.path.join(tmp, "feats.ark"), "wb") as f:
        kaldi_io.write_mat(f, (rs.randn(frames, 30) + tilt + 3.0).astype(np.float32), key="rec1")
    with open(os.path.join(tmp, "reco2num_spk"), "w") as f:
        f.write("rec1 1\n")
    windows = D.subsegments(0, frames, 150, 75, 50)
    assert len(windows) == 39
    scorer = _scorer()

    def run(stop_args, tag, **stop):
        emb, rttm = os.path.join(tmp, tag + ".ark"), os.path.join(tmp, tag + ".rttm")
        _diarize(stop_args + ["--first-pass-max-points", "16", "--write-embeddings", emb, model, "ark:" + os.path.join(tmp, "feats.ark"), rttm])
        got = open(rttm).read().splitlines()
        assert got and all(RTTM_LINE.match(ln) for ln in got)
        vecs = dict(kaldi_io.read_vec_flt_ark(emb))
        s = scorer.dense(scorer.prepare(np.stack([vecs["rec1-%07d-%07d" % w] for w in windows]))).cpu().numpy()
        labels, first, second, bounds = R2.two_pass(s, first_pass_max_points=16, **stop)
        assert bounds == [0, 13, 26, 39]
        assert got == ["SPEAKER rec1 0 %.3f %.3f <NA> <NA> %d <NA> <NA>" % (a * 0.01, (b - a) * 0.01, l + 1) for a, b, l in D.rttm_turns(windows, labels)]
        return s, first, second

    # one speaker asked for: every subset stops at ten clusters, the second pass merges the thirty
    s, first, second = run(["--reco2num-spk", os.path.join(tmp, "reco2num_spk")], "num", target=1)
    assert [len(m) for m, _ in first] == [3, 3, 3] and len(second[0]) == 29
    # a threshold among the second pass's merge values: whatever it stops, the driver and the restatement stop alike
    v = np.sort(second[1])[::-1]
    threshold = 0.5 * (float(v[9]) + float(v[10]))
    run(["--threshold", repr(threshold)], "thr", threshold=threshold)
