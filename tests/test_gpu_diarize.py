"""Diarization end to end on a real MI355X: Diarizer (prepare -> dense -> ahc_cluster) on synthetic embeddings behind a back end trained
on drawn speakers, and nnet/lib/diarize.py on synthetic features with a freshly initialised model - its RTTM against what the window
planner, the driver's own written embeddings, the scorer's dense matrix and the float32 restatement of the clusterer give."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import ahc_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "tf_kaldi_speaker_amd")
DEV = "cuda:0"
D_EMB, LDA_DIM = 24, 10
RTTM_LINE = re.compile(r"^SPEAKER (\S+) 0 (\d+\.\d{3}) (\d+\.\d{3}) <NA> <NA> (\d+) <NA> <NA>$")


def _first_appearance(labels):
    """Labels renumbered in order of first appearance - the clusterer's numbering (ascending smallest member)."""
    seen = {}
    return [seen.setdefault(int(l), len(seen)) for l in labels]


_WORLD = {}


def _world():
    """A back end trained on 40 drawn speakers, and three recordings of 2 - 4 new, well separated speakers; built once."""
    if not _WORLD:
        from tf_kaldi_speaker_amd.misc import backend as B
        rs = np.random.RandomState(5)
        basis = rs.randn(LDA_DIM, D_EMB)      # the speakers live in a 10-dimensional subspace; the noise fills all 24
        draw = lambda spk: spk @ basis + 0.15 * rs.randn(spk.shape[0], D_EMB) + 0.5
        spk = rs.randn(40, LDA_DIM)
        train = draw(np.repeat(spk, 8, axis=0)).astype(np.float32)
        keys = ["u%03d" % i for i in range(len(train))]
        spk2utt = [("s%02d" % s, keys[8 * s:8 * s + 8]) for s in range(40)]
        _WORLD["backend"] = B.Backend.train(train, keys, spk2utt, lda_dim=LDA_DIM, device=DEV)
        recos = {}
        for name, n, k in (("recA", 30, 2), ("recB", 45, 3), ("recC", 61, 4)):
            who = rs.randint(0, k, n)
            who[:k] = np.arange(k)      # every speaker speaks
            recos[name] = (draw(2.0 * rs.randn(k, LDA_DIM)[who]).astype(np.float32), who)
        _WORLD["recos"] = recos
    return _WORLD["backend"], _WORLD["recos"]


@pytest.mark.parametrize("mode", ["cosine", "lda_cos", "plda"])
def test_diarizer_finds_the_true_partition(mode):
    from tf_kaldi_speaker_amd.misc import backend as B
    from tf_kaldi_speaker_amd.misc import diarization as D
    from tf_kaldi_speaker_amd.misc import scoring as S
    backend, recos = _world()
    scorer = S.CosineScorer(DEV, center=backend.mean) if mode == "cosine" else B.BackendScorer(backend, mode, DEV)
    emb = {k: x for k, (x, _) in recos.items()}
    truth = {k: _first_appearance(who) for k, (_, who) in recos.items()}
    # with the number of speakers
    got = D.Diarizer(scorer, reco2num_spk={k: int(who.max()) + 1 for k, (_, who) in recos.items()}).cluster(emb)
    assert list(got) == list(emb) and {k: v.tolist() for k, v in got.items()} == truth
    # with a threshold between the two score populations: every average of same-speaker scores is above it, every other one below
    lo, hi = -np.inf, np.inf
    for k, (x, who) in recos.items():
        s = scorer.dense(scorer.prepare(x)).cpu().numpy()
        same = np.equal.outer(who, who)
        upper = np.triu(np.ones_like(same), 1)
        lo, hi = max(lo, s[~same & upper].max()), min(hi, s[same & upper].min())
    assert lo < hi, (mode, lo, hi)
    diar = D.Diarizer(scorer, threshold=0.5 * (float(lo) + float(hi)))
    got = diar.cluster(emb)
    assert {k: v.tolist() for k, v in got.items()} == truth
    # one recording per call: a workspace that holds the largest recording only gives the same labels
    scorer.workspace_bytes = 4 * (61 * 64 + 61 * 61)
    assert {k: v.tolist() for k, v in diar.cluster(emb).items()} == truth
    scorer.workspace_bytes -= 4
    with pytest.raises(ValueError, match="recording recC needs 30500 bytes of scores, the workspace holds 30496"):
        diar.cluster(emb)
    # DER 0 through the turns
    for k, (_, who) in recos.items():
        windows = D.subsegments(0, 75 * (len(who) + 1), 150, 75, 50)
        assert len(windows) == len(who)
        turns = lambda labels: [(0.01 * s, 0.01 * e, l) for s, e, l in D.rttm_turns(windows, labels)]
        assert D.der(turns(who), turns(got[k])) == (0.0, 0.0, 0.0, 0.0)
    with pytest.raises(ValueError, match="no number of speakers for recording recB"):
        D.Diarizer(scorer, reco2num_spk={"recA": 2}).cluster({"recA": emb["recA"], "recB": emb["recB"]})


def _model(model):
    """A toy model directory: random weights, moving statistics away from (0, 1)."""
    from tf_kaldi_speaker_amd.model.trainer import Trainer
    from tf_kaldi_speaker_amd.misc.utils import Params
    nnet = os.path.join(model, "nnet")
    os.makedirs(nnet)
    cfg = {"network_type": "tdnn", "loss_func": "softmax", "pooling_type": "statistics_pooling", "embedding_node": "tdnn6_dense", "seed": 0,
           "last_layer_no_bn": False, "last_layer_linear": False, "weight_l2_regularizer": 1e-2, "batchnorm_momentum": 0.99,
           "optimizer": "sgd", "num_nodes_pooling_layer": 1500, "num_nodes_last_layer": 512, "feature_norm": False, "precision": "f32"}
    json.dump(cfg, open(os.path.join(nnet, "config.json"), "w"))
    open(os.path.join(nnet, "feature_dim"), "w").write("30\n")
    tr = Trainer(Params(os.path.join(nnet, "config.json")), model, single_cpu=True)
    tr.build("predict", dim=30)
    V = tr.engine.get_variables()
    rs = np.random.RandomState(7)
    for k in V:
        if k.endswith("moving_mean"):
            V[k] = (rs.randn(*V[k].shape) * 0.1).astype(np.float32)
        if k.endswith("moving_variance"):
            V[k] = (0.5 + rs.rand(*V[k].shape)).astype(np.float32)
    np.savez(os.path.join(nnet, "model-1.npz"), **V)
    open(os.path.join(nnet, "checkpoint"), "w").write('model_checkpoint_path: "model-1"\nall_model_checkpoint_paths: "model-1"\n')
    tr.close()


def _diarize(args, ok=True):
    env = dict(os.environ, TF_KALDI_ROOT=PKG, PYTHONPATH=PKG)
    r = subprocess.run([sys.executable, os.path.join(PKG, "nnet", "lib", "diarize.py")] + args, env=env, cwd=PKG, capture_output=True, text=True, timeout=600)
    assert (r.returncode == 0) == ok, r.stderr[-3000:]
    return r.stderr


def _expected_rttm(windows, emb_ark, stop):
    """The RTTM lines the planner's windows, the written embeddings, CosineScorer.dense and the float32 restatement give; stop(reco) -> the
    restatement's stop arguments.  Also -> {recording: merge values of the full run}."""
    from tf_kaldi_speaker_amd.dataset import kaldi_io
    from tf_kaldi_speaker_amd.misc import diarization as D
    from tf_kaldi_speaker_amd.misc import scoring as S
    vecs = dict(kaldi_io.read_vec_flt_ark(emb_ark))
    assert list(vecs) == ["%s-%07d-%07d" % (reco, s, e) for reco, ws in windows.items() for s, e in ws]      # keys, in order
    scorer = S.CosineScorer(DEV)
    lines, values = [], {}
    for reco, ws in windows.items():
        x = np.stack([vecs["%s-%07d-%07d" % (reco, s, e)] for s, e in ws])
        s = scorer.dense(scorer.prepare(x)).cpu().numpy()
        labels = R.cluster(s, **stop(reco))[0]
        values[reco] = R.cluster(s, target=1)[2]
        for a, b, l in D.rttm_turns(ws, labels):
            lines.append("SPEAKER %s 0 %.3f %.3f <NA> <NA> %d <NA> <NA>" % (reco, a * 0.01, (b - a) * 0.01, l + 1))
    return lines, values


def test_driver_end_to_end(tmp_path):
    from tf_kaldi_speaker_amd.dataset import kaldi_io
    from tf_kaldi_speaker_amd.misc import diarization as D
    tmp = str(tmp_path)
    model = os.path.join(tmp, "exp")
    _model(model)
    rs = np.random.RandomState(17)
    # two recordings whose halves differ in their spectral tilt, so that a random network separates them somewhat
    feats, vads = {}, {}
    for reco, frames in (("rec1", 700), ("rec2", 460)):
        tilt = np.where(np.arange(frames)[:, None] < frames // 2, np.linspace(-2, 2, 30)[None, :], np.linspace(2, -2, 30)[None, :])
        feats[reco] = (rs.randn(frames, 30) + tilt + 3.0).astype(np.float32)
        vads[reco] = np.ones(frames, np.float32)
    vads["rec1"][300:330] = 0      # two speech segments: [0, 300) and [330, 700)
    vads["rec2"][:20] = 0          # [20, 460)
    vads["rec2"][440:452] = 0      # ... cut into [20, 440) and [452, 460): 8 frames, dropped
    with open(os.path.join(tmp, "feats.ark"), "wb") as f:
        for reco, m in feats.items():
            kaldi_io.write_mat(f, m, key=reco)
    with open(os.path.join(tmp, "vad.ark"), "wb") as f:
        for reco, v in vads.items():
            kaldi_io.write_vec_flt(f, v, key=reco)
    with open(os.path.join(tmp, "reco2num_spk"), "w") as f:
        f.write("rec1 2\nrec2 3\n")
    windows = {reco: [w for s, e in D.speech_segments(vads[reco]) for w in D.subsegments(s, e, 150, 75, 50)] for reco in feats}
    assert windows["rec1"][:4] == [(0, 150), (75, 225), (150, 300), (330, 480)] and windows["rec2"][-1] == (320, 440)
    common = ["--vad", "ark:" + os.path.join(tmp, "vad.ark"), model, "ark:" + os.path.join(tmp, "feats.ark")]

    def run(stop_args, stop, tag):
        emb, rttm = os.path.join(tmp, tag + ".ark"), os.path.join(tmp, tag + ".rttm")
        stderr = _diarize(stop_args + ["--write-embeddings", emb] + common + [rttm])
        got = open(rttm).read().splitlines()
        assert got and all(RTTM_LINE.match(ln) for ln in got), got[:3]
        want, values = _expected_rttm(windows, emb, stop)
        assert got == want
        assert "Segment 452 .. 460: 8 frames, fewer than 50, dropped" in stderr
        return got, values

    got, values = run(["--reco2num-spk", os.path.join(tmp, "reco2num_spk")], lambda reco: dict(target={"rec1": 2, "rec2": 3}[reco]), "num")
    assert {reco: len({ln.split()[7] for ln in got if ln.split()[1] == reco}) for reco in feats} == {"rec1": 2, "rec2": 3}
    # a threshold that stops rec1 midway: between two of its merge values
    v = values["rec1"]
    k = len(v) // 2
    assert v[k + 1] < v[k]
    threshold = 0.5 * (float(v[k]) + float(v[k + 1]))
    got, _ = run(["--threshold", repr(threshold)], lambda reco: dict(threshold=threshold), "thr")
    assert len({ln.split()[7] for ln in got if ln.split()[1] == "rec1"}) == len(windows["rec1"]) - (k + 1)


def test_driver_refusals(tmp_path):
    tail = [str(tmp_path / "exp"), "ark:" + str(tmp_path / "feats.ark"), str(tmp_path / "out.rttm")]
    for args, what in (([], "exactly one of --threshold and --reco2num-spk"),
                       (["--threshold", "0.1", "--reco2num-spk", "x"], "exactly one of --threshold and --reco2num-spk"),
                       (["--threshold", "0.1", "--segments", "s", "--vad", "ark:v"], "--segments and --vad: both name the speech"),
                       (["--threshold", "0.1", "--scoring", "plda"], "--scoring plda needs --backend DIR")):
        assert what in _diarize(args + tail, ok=False)
