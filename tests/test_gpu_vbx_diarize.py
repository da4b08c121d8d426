"""VBx behind the clusterer, end to end on a real MI355X: Diarizer(vbx=...) on the synthetic recordings of tests/test_gpu_diarize.py from a
threshold that over-splits them, the re-clustering down to 32 speakers, and nnet/lib/diarize.py --vbx - its RTTM against what the window
planner, the driver's own written embeddings, the scorer's dense matrix, the float32 restatement of the clusterer, plda_space, vbx_init,
ops.vbx and rttm_turns give; without --vbx the driver writes what it wrote before."""
import logging
import os

import numpy as np
import pytest

from tests import ahc_ref as A
from tests import test_gpu_diarize as TD

pytestmark = pytest.mark.gpu

DEV = TD.DEV


def _scorer():
    from tf_kaldi_speaker_amd.misc import backend as B
    backend, recos = TD._world()
    return B.BackendScorer(backend, "plda", DEV), recos


def _oversplitting_threshold(scorer, recos):
    """A threshold above three tenths of the same-speaker scores of every recording: the clusterer stops with every speaker in several pieces."""
    cut = -np.inf
    for x, who in recos.values():
        s = scorer.dense(scorer.prepare(x)).cpu().numpy()
        same = np.equal.outer(who, who) & (np.triu(np.ones((len(who), len(who)), bool), 1))
        cut = max(cut, float(np.quantile(s[same], 0.3)))
    return cut


def test_diarizer_with_vbx_finds_the_true_partition():
    from tf_kaldi_speaker_amd.misc import diarization as D
    scorer, recos = _scorer()
    emb = {k: x for k, (x, _) in recos.items()}
    truth = {k: TD._first_appearance(who) for k, (_, who) in recos.items()}
    threshold = _oversplitting_threshold(scorer, recos)
    plain = D.Diarizer(scorer, threshold=threshold).cluster(emb)
    for k, (_, who) in recos.items():
        assert int(plain[k].max()) + 1 > int(who.max()) + 1, (k, int(plain[k].max()) + 1)      # the start is over-split
    diar = D.Diarizer(scorer, threshold=threshold, vbx=D.VbxOptions())
    got = diar.cluster(emb)
    assert list(got) == list(emb) and {k: v.tolist() for k, v in got.items()} == truth
    for k, (before, after, iters, elbo) in diar.vbx_report.items():
        assert before == min(int(plain[k].max()) + 1, 32) and after == int(recos[k][1].max()) + 1 and 2 <= iters <= 20 and np.isfinite(elbo)
    # one recording per call gives the same labels; vbx=None is the clusterer alone
    scorer.workspace_bytes = 115800      # recC's rows, start and scratch at 32 speakers: the largest of the three, and no two fit together
    assert {k: v.tolist() for k, v in diar.cluster(emb).items()} == truth
    scorer.workspace_bytes -= 4
    with pytest.raises(ValueError, match="recording recC needs 115800 bytes of scores, the workspace holds 115796"):
        diar.cluster(emb)
    scorer.workspace_bytes = 1 << 30
    assert {k: v.tolist() for k, v in D.Diarizer(scorer, threshold=threshold, vbx=None).cluster(emb).items()} == {k: v.tolist() for k, v in plain.items()}
    # a scorer without a PLDA space is refused by name
    from tf_kaldi_speaker_amd.misc import scoring as S
    with pytest.raises(ValueError, match="Diarizer: VBx needs a BackendScorer in the plda mode"):
        D.Diarizer(S.CosineScorer(DEV), threshold=0.0, vbx=D.VbxOptions())
    from tf_kaldi_speaker_amd.misc import backend as B
    with pytest.raises(ValueError, match="BackendScorer.plda_space: needs a PLDA model and the plda mode"):
        D.Diarizer(B.BackendScorer(TD._world()[0], "lda_cos", DEV), threshold=0.0, vbx=D.VbxOptions()).cluster(emb)


def test_more_than_32_clusters_are_clustered_once_more(caplog):
    from tf_kaldi_speaker_amd.misc import diarization as D
    scorer, recos = _scorer()
    emb = {k: x for k, (x, _) in recos.items()}
    opts = D.VbxOptions()
    diar = D.Diarizer(scorer, threshold=1e30, vbx=opts)      # nothing merges: 30, 45 and 61 clusters
    with caplog.at_level(logging.INFO, logger="tf_kaldi_speaker_amd"):
        got = diar.cluster(emb)
    lines = [r.getMessage() for r in caplog.records if "clustered once more" in r.getMessage()]
    assert lines == ["[INFO] Recording recB, recC: more than 32 clusters, clustered once more down to 32 for VBx."]
    assert {k: v[0] for k, v in diar.vbx_report.items()} == {"recA": 30, "recB": 32, "recC": 32}
    want = D.Diarizer(scorer, reco2num_spk={"recA": 30, "recB": 32, "recC": 32}, vbx=opts).cluster(emb)      # the same start, stated as targets
    assert {k: v.tolist() for k, v in got.items()} == {k: v.tolist() for k, v in want.items()}
    for k, v in got.items():
        assert v.tolist() == TD._first_appearance(v) and int(v.max()) + 1 == diar.vbx_report[k][1] <= diar.vbx_report[k][0]


def _backend_dir(path, emb_ark):
    """A back end for the driver's own window embeddings, written down rather than trained (a few dozen near-equal vectors of a random
    network train no PLDA model): their mean, their first six principal directions as the LDA, a PLDA model with a scaled unit transform
    and psi falling from 6 to 0.5."""
    from tf_kaldi_speaker_amd.dataset import kaldi_io
    from tf_kaldi_speaker_amd.misc import backend as B
    x = np.stack([v for _, v in kaldi_io.read_vec_flt_ark(emb_ark)]).astype(np.float64)
    mean = x.mean(axis=0)
    directions = np.linalg.svd(x - mean, full_matrices=False)[2][:6]
    lda = np.concatenate([directions, np.zeros((6, 1))], axis=1)
    be = B.Backend(mean, lda, dict(mean=np.zeros(6), transform=1.5 * np.eye(6), psi=np.linspace(6.0, 0.5, 6)))
    be.save(path)
    return B.Backend.load(path)


def test_driver_with_and_without_vbx(tmp_path):
    import torch
    from tf_kaldi_speaker_amd import ops
    from tf_kaldi_speaker_amd.dataset import kaldi_io
    from tf_kaldi_speaker_amd.misc import backend as B
    from tf_kaldi_speaker_amd.misc import diarization as D
    tmp = str(tmp_path)
    model = os.path.join(tmp, "exp")
    TD._model(model)
    rs = np.random.RandomState(23)
    feats = {}
    for reco, frames in (("rec1", 1800), ("rec2", 1300)):
        tilt = np.where(np.arange(frames)[:, None] < frames // 2, np.linspace(-2, 2, 30)[None, :], np.linspace(2, -2, 30)[None, :])
        feats[reco] = (rs.randn(frames, 30) + tilt + 3.0).astype(np.float32)
    with open(os.path.join(tmp, "feats.ark"), "wb") as f:
        for reco, m in feats.items():
            kaldi_io.write_mat(f, m, key=reco)
    windows = {reco: D.subsegments(0, m.shape[0], 150, 75, 50) for reco, m in feats.items()}
    tail = [model, "ark:" + os.path.join(tmp, "feats.ark")]
    emb0 = os.path.join(tmp, "emb0.ark")
    TD._diarize(["--threshold", "0.5", "--write-embeddings", emb0] + tail + [os.path.join(tmp, "cos.rttm")])
    bdir = os.path.join(tmp, "backend")
    be = _backend_dir(bdir, emb0)
    scorer = B.BackendScorer(be, "plda", DEV)

    def expected(emb_ark, threshold, opts):
        vecs = dict(kaldi_io.read_vec_flt_ark(emb_ark))
        lines, report = [], {}
        for reco, ws in windows.items():
            x = np.stack([vecs["%s-%07d-%07d" % (reco, s, e)] for s, e in ws])
            labels = A.cluster(scorer.dense(scorer.prepare(x)).cpu().numpy(), threshold=threshold)[0]
            if opts is not None:
                k = int(labels.max()) + 1
                assert 1 < k <= 32
                rows, psi = scorer.plda_space(x)
                out = ops.vbx(rows.reshape(-1), [0], [len(ws)], be.dim, psi, torch.from_numpy(D.vbx_init(labels, k, opts.init_smoothing).ravel()).to(DEV),
                              torch.full((k,), 1.0 / k, device=DEV), [k], ld=[rows.shape[1]], loop_prob=opts.loop_prob, fa=opts.fa, fb=opts.fb,
                              max_iters=opts.max_iters, epsilon=opts.epsilon)
                n_iters = int(out[3][0])
                labels = np.asarray(TD._first_appearance(out[4].cpu().numpy()))
                report[reco] = (k, int(labels.max()) + 1, n_iters, float(out[2][0, n_iters - 1]))
            for a, b, l in D.rttm_turns(ws, labels):
                lines.append("SPEAKER %s 0 %.3f %.3f <NA> <NA> %d <NA> <NA>" % (reco, a * 0.01, (b - a) * 0.01, l + 1))
        return "".join(ln + "\n" for ln in lines), report

    # a threshold midway through rec1's merges: several clusters per recording are left for VBx
    x1 = np.stack([dict(kaldi_io.read_vec_flt_ark(emb0))["rec1-%07d-%07d" % w] for w in windows["rec1"]])
    values = A.cluster(scorer.dense(scorer.prepare(x1)).cpu().numpy(), target=1)[2]
    k = len(values) - 5
    assert values[k + 1] < values[k]
    threshold = 0.5 * (float(values[k]) + float(values[k + 1]))
    common = ["--backend", bdir, "--scoring", "plda", "--threshold", repr(threshold)]
    # without --vbx: the bytes the clusterer alone gives, and no word of VBx in the log
    emb, rttm = os.path.join(tmp, "plain.ark"), os.path.join(tmp, "plain.rttm")
    stderr = TD._diarize(common + ["--write-embeddings", emb] + tail + [rttm])
    want, _ = expected(emb, threshold, None)
    assert open(rttm).read() == want and want and "VBx" not in stderr
    # with --vbx
    opts = D.VbxOptions(fa=0.4, fb=11.0, loop_prob=0.95, max_iters=12, epsilon=1e-3, init_smoothing=4.0)
    emb, rttm = os.path.join(tmp, "vbx.ark"), os.path.join(tmp, "vbx.rttm")
    stderr = TD._diarize(common + ["--vbx", "--vbx-fa", "0.4", "--vbx-fb", "11", "--vbx-loop-prob", "0.95", "--vbx-max-iters", "12", "--vbx-epsilon", "1e-3",
                                   "--vbx-init-smoothing", "4", "--write-embeddings", emb] + tail + [rttm])
    want, report = expected(emb, threshold, opts)
    assert open(rttm).read() == want and want
    for reco, (before, after, iters, elbo) in report.items():
        assert "Recording %s: VBx: %d speakers before, %d after, %d iterations, last ELBO %.6f." % (reco, before, after, iters, elbo) in stderr
    assert report["rec1"][0] == len(windows["rec1"]) - (k + 1) == 5


def test_driver_refuses_vbx_without_plda(tmp_path):
    tail = [str(tmp_path / "exp"), "ark:" + str(tmp_path / "feats.ark"), str(tmp_path / "out.rttm")]
    for args, what in ((["--threshold", "0.1", "--vbx"], "--vbx needs --scoring plda"),
                       (["--threshold", "0.1", "--vbx", "--backend", "b", "--scoring", "lda_cos"], "--vbx needs --scoring plda"),
                       (["--threshold", "0.1", "--vbx", "--backend", "b", "--scoring", "plda", "--vbx-loop-prob", "1"], "--vbx-loop-prob must lie strictly between 0 and 1"),
                       (["--threshold", "0.1", "--vbx", "--backend", "b", "--scoring", "plda", "--vbx-max-iters", "65"], "--vbx-max-iters lie in 1 .. 64")):
        assert what in TD._diarize(args + tail, ok=False)
