"""Threshold tuning end to end on a real MI355X: Diarizer.sweep against Diarizer.cluster run once per threshold (label for label: one
merge log and its cuts must give what the clusterer gives when it is run with each threshold), DerSweep's pooled table against
rttm_turns plus the restatement of tests/diar_eval_ref.py (integers: equal), and nnet/lib/tune_diarization.py on two-speaker
recordings whose score populations leave a gap: the threshold it writes lies in the gap and diarize.py reaches DER 0 with it."""
import logging
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import diar_eval_ref as R
from tests import test_gpu_diarize as TD

pytestmark = pytest.mark.gpu

DEV = TD.DEV
PKG = TD.PKG


def _recordings():
    """The three synthetic recordings of tests/test_gpu_diarize.py (30, 45 and 61 windows) and a fourth of 150 windows made of their rows."""
    backend, recos = TD._world()
    emb = {k: x for k, (x, _) in recos.items()}
    emb["recL"] = np.concatenate([emb["recA"], emb["recB"], emb["recC"], emb["recA"][:14]])
    return backend, emb


def _thresholds(scorer, emb, target_energy=None):
    """Eleven thresholds over the range of a recording's scores (its 2 % .. 98 % quantiles; with target_energy the scores behind its own
    PCA, as the Diarizer takes them), one above and one below every score."""
    if target_energy is None:
        s = scorer.dense(scorer.prepare(emb["recC"])).cpu().numpy()
    else:
        prepared, model = scorer.prepare_pca([emb["recC"]], target_energy)[0]
        s = scorer.dense(prepared, model=model).cpu().numpy()
    upper = s[np.triu_indices(s.shape[0], 1)]
    return [-1e30] + [float(q) for q in np.quantile(upper, np.linspace(0.02, 0.98, 9))] + [1e30]


def _same(got, want, where):
    assert list(got) == list(want)
    for k in want:
        assert got[k].dtype == np.int32 and got[k].tolist() == want[k].tolist(), (where, k)


@pytest.mark.parametrize("mode", ["cosine", "plda", "plda_vbx", "plda_pca", "plda_two_pass", "plda_vbx_two_pass"])
def test_sweep_equals_cluster_run_with_each_threshold(mode, caplog):
    from tf_kaldi_speaker_amd.misc import backend as B
    from tf_kaldi_speaker_amd.misc import diarization as D
    from tf_kaldi_speaker_amd.misc import scoring as S
    backend, emb = _recordings()
    scorer = S.CosineScorer(DEV, center=backend.mean) if mode == "cosine" else B.BackendScorer(backend, "plda", DEV)
    options = {}
    if "vbx" in mode:
        options["vbx"] = D.VbxOptions()
    if "pca" in mode:
        options["target_energy"] = 0.9
    if "two_pass" in mode:
        options["first_pass_max_points"] = 64      # recL (150 windows) takes the two passes, recA - recC beside it one log
    else:
        emb = {k: v for k, v in emb.items() if k != "recL"}
    thresholds = _thresholds(scorer, emb, options.get("target_energy"))
    with caplog.at_level(logging.INFO, logger="tf_kaldi_speaker_amd"):
        got = D.Diarizer(scorer, threshold=0.0, **options).sweep(emb, thresholds)
    said = [r.getMessage() for r in caplog.records if "no single merge log" in r.getMessage()]
    assert said == (["[INFO] Recording recL: more than 64 windows, no single merge log: clustered in two passes once per threshold (11 times)."] if "two_pass" in mode else [])
    assert all(got[k].shape == (len(thresholds), emb[k].shape[0]) for k in emb)
    for i, threshold in enumerate(thresholds):
        want = D.Diarizer(scorer, threshold=threshold, **options).cluster(emb)
        _same({k: v[i] for k, v in got.items()}, want, (mode, threshold))
    if "vbx" not in mode:      # the thresholds do span the log: from one cluster to a cluster per window
        counts = [int(got["recC"][i].max()) + 1 for i in range(len(thresholds))]
        assert counts[0] == 1 and counts[-1] == 61 and len(set(counts)) >= 4, counts
    if mode == "plda_vbx":
        # a grid of VBx options over the same cuts: each entry is what a Diarizer with those options gives
        grid = [D.VbxOptions(fa=0.2, fb=10.0), D.VbxOptions(loop_prob=0.9)]
        swept = D.Diarizer(scorer, threshold=0.0, vbx=grid[0]).sweep(emb, thresholds[3:6], vbx_grid=grid)
        for j, opt in enumerate(grid):
            for i, threshold in enumerate(thresholds[3:6]):
                _same({k: v[j, i] for k, v in swept.items()}, D.Diarizer(scorer, threshold=threshold, vbx=opt).cluster(emb), (j, threshold))
    if mode == "cosine":
        with pytest.raises(ValueError, match="^Diarizer: sweep takes a non-empty list of thresholds, none of them NaN$"):
            D.Diarizer(scorer, threshold=0.0).sweep(emb, [0.1, float("nan")])
        with pytest.raises(ValueError, match="^Diarizer: vbx_grid needs a Diarizer with vbx and at least one entry$"):
            D.Diarizer(scorer, threshold=0.0).sweep(emb, [0.1], vbx_grid=[D.VbxOptions()])


@pytest.mark.parametrize("collar,overlap", [(0.25, "score"), (0.0, "first"), (0.1, "ignore")])
def test_pooled_der_table_equals_rttm_turns_plus_the_restatement(collar, overlap):
    from tf_kaldi_speaker_amd.misc import diarization as D
    from tf_kaldi_speaker_amd.misc import scoring as S
    backend, recos = TD._world()
    scorer = S.CosineScorer(DEV, center=backend.mean)
    emb = {k: x for k, (x, _) in recos.items()}
    thresholds = _thresholds(scorer, emb)
    labels = D.Diarizer(scorer, threshold=0.0).sweep(emb, thresholds)
    # the reference: the true turns with their boundaries moved, a second speaker over some of them, and silence where windows are
    rs = np.random.RandomState(31)
    windows, reference = {}, {}
    for k, (_, who) in recos.items():
        windows[k] = [(0.01 * s, 0.01 * e) for s, e in D.subsegments(0, 75 * (len(who) + 1), 150, 75, 50)]
        turns = [(max(s + rs.uniform(-0.3, 0.3), 0.0), e + rs.uniform(-0.3, 0.3), "spk%d" % l) for s, e, l in D.rttm_turns(windows[k], who)]
        turns = [t for t in turns if t[1] > t[0]][:-2] + [(3.0, 7.5, "guest"), (turns[-1][1] + 1.0, turns[-1][1] + 2.0, "spk0")]
        reference[k] = turns
    table = D.DerSweep(DEV, reference, windows, collar=collar, overlap=overlap).score(labels)
    want = np.zeros((len(thresholds), len(recos), 4), np.int64)
    for i, k in enumerate(recos):
        frames = int(round(max([e for _, e, _ in reference[k]] + [e for _, e in windows[k]]) / R.FRAME))
        mask, scored, speakers = R.reference(reference[k], frames, collar, overlap)
        for c in range(len(thresholds)):
            h = R.hypothesis(D.rttm_turns(windows[k], labels[k][c]), frames)
            speech, miss, fa, shared = R.confusion(mask, scored, np.where(h >= 0, np.arange(frames), -1), np.maximum(h, 0), speakers, int(h.max()) + 1)
            want[c, i] = speech, miss, fa, R.speaker_error(speech, miss, shared)
    assert (table.status == 0).all() and table.keys == list(recos)
    for got, j in ((table.speech, 0), (table.miss, 1), (table.fa, 2), (table.error, 3)):
        assert got.dtype == np.int64 and np.array_equal(got, want[..., j]), j
    assert want[..., 1].min() > 0 and want[..., 2].min() > 0 and want[..., 3].max() > 0      # (every kind of error occurs)
    for c in range(len(thresholds)):
        speech, parts = int(want[c, :, 0].sum()), [int(want[c, :, j].sum()) for j in (1, 2, 3)]
        assert table.pooled(c) == tuple(p / speech for p in parts) + (sum(parts) / speech,)
    # a cut with more clusters than are counted has no DER, and says why
    many = {k: np.stack([v[0], np.arange(v.shape[1], dtype=np.int32)]) for k, v in labels.items()}
    wide = dict(many, recW=np.stack([np.zeros(300, np.int32), np.arange(300, dtype=np.int32)]))
    sweep = D.DerSweep(DEV, dict(reference, recW=[(0.0, 5.0, "a")]), dict(windows, recW=[(0.01 * i, 0.01 * i + 1.5) for i in range(300)]), collar=collar, overlap=overlap)
    table = sweep.score(wide)
    assert table.pooled(0) is not None and table.pooled(1) is None and table.why_not(1) == "recording recW has 300 clusters, 256 are counted"
    with pytest.raises(ValueError, match="^DerSweep: recording recQ has windows but no reference$"):
        D.DerSweep(DEV, reference, dict(windows, recQ=[(0.0, 1.5)]))


def _run(script, args):
    env = dict(os.environ, TF_KALDI_ROOT=PKG, PYTHONPATH=PKG)
    r = subprocess.run([sys.executable, os.path.join(PKG, "nnet", "lib", script)] + args, env=env, cwd=PKG, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stderr


def test_driver_writes_a_threshold_inside_the_gap_and_diarize_reaches_der_zero_with_it(tmp_path):
    from tf_kaldi_speaker_amd.dataset import kaldi_io
    from tf_kaldi_speaker_amd.misc import diarization as D
    from tf_kaldi_speaker_amd.misc import scoring as S
    tmp = str(tmp_path)
    model = os.path.join(tmp, "exp")
    TD._model(model)
    rs = np.random.RandomState(41)
    # two recordings of two speakers with opposite spectral tilts, one speech segment each: every window holds one speaker
    speech = {"rec1": [(0, 600), (650, 1250)], "rec2": [(40, 500), (520, 1000)]}
    tilt = np.linspace(-2, 2, 30)[None, :]
    feats = {}
    for reco, ((a0, a1), (b0, b1)) in speech.items():
        x = rs.randn(b1 + 30, 30)
        x[:a1] += tilt
        x[a1:] -= tilt
        feats[reco] = (x + 3.0).astype(np.float32)
    with open(os.path.join(tmp, "feats.ark"), "wb") as f:
        for reco, m in feats.items():
            kaldi_io.write_mat(f, m, key=reco)
    with open(os.path.join(tmp, "segments"), "w") as f, open(os.path.join(tmp, "ref.rttm"), "w") as g:
        for reco, spans in speech.items():
            for who, (s, e) in zip("AB", spans):
                f.write("%s-%s %s %.2f %.2f\n" % (reco, who, reco, 0.01 * s, 0.01 * e))
                g.write("SPEAKER %s 0 %.3f %.3f <NA> <NA> %s <NA> <NA>\n" % (reco, 0.01 * s, 0.01 * (e - s), who))
    with open(os.path.join(tmp, "reco2num_spk"), "w") as f:
        f.write("rec1 2\nrec2 2\n")
    common = ["--cmn-window", "0", "--segments", os.path.join(tmp, "segments"), model, "ark:" + os.path.join(tmp, "feats.ark")]
    emb_ark = os.path.join(tmp, "emb.ark")
    _run("diarize.py", ["--reco2num-spk", os.path.join(tmp, "reco2num_spk"), "--write-embeddings", emb_ark] + common + [os.path.join(tmp, "num.rttm")])
    # the gap between the two score populations: every same-speaker score above every other one, over both recordings
    vecs = list(kaldi_io.read_vec_flt_ark(emb_ark))
    scorer, lo, hi = S.CosineScorer(DEV), -np.inf, np.inf
    for reco, spans in speech.items():
        rows = [(key, v) for key, v in vecs if key.startswith(reco + "-")]
        who = np.asarray([int(key.rsplit("-", 2)[1]) >= spans[1][0] for key, _ in rows])
        assert 5 <= who.sum() < len(who) - 5
        s = scorer.dense(scorer.prepare(np.stack([v for _, v in rows]))).cpu().numpy()
        same, upper = np.equal.outer(who, who), np.triu(np.ones((len(who), len(who)), bool), 1)
        lo, hi = max(lo, float(s[~same & upper].max())), min(hi, float(s[same & upper].min()))
    assert lo + 1e-3 < hi, (lo, hi)
    mid = 0.5 * (lo + hi)
    out = os.path.join(tmp, "tune")
    stderr = _run("tune_diarization.py", ["--thresholds", "-1.5,%r,%r,2.0" % (mid, 0.5 * (mid + hi)), "--ref-rttm", os.path.join(tmp, "ref.rttm"), "ark:" + emb_ark, out])
    written = open(os.path.join(out, "threshold")).read()
    assert float(written) == mid and lo < float(written) < hi      # the lower of the two thresholds in the gap: a tie goes to it
    table = open(os.path.join(out, "der_table.txt")).read().splitlines()
    assert len(table) == 4 and table[1] == "threshold %r miss 0.00 fa 0.00 error 0.00 DER 0.00" % mid and table[2].endswith("DER 0.00")
    assert not table[0].endswith("DER 0.00") and not table[3].endswith("DER 0.00")      # one cluster; a cluster per window
    assert "2 recordings, 4 grid points; the best: threshold %r miss 0.00" % mid in stderr
    _run("diarize.py", ["--threshold", written.strip()] + common + [os.path.join(tmp, "thr.rttm")])
    hyp, ref = D.read_rttm(os.path.join(tmp, "thr.rttm")), D.read_rttm(os.path.join(tmp, "ref.rttm"))
    assert list(hyp) == list(ref)
    for reco in ref:
        assert D.der(ref[reco], hyp[reco]) == (0.0, 0.0, 0.0, 0.0), reco
