"""The feature front end inside batched extraction on a real MI355X: Trainer.predict_batch(cmn_window=, voiced=) and nnet/lib/extract.py
--cmn-window / --vad on RAW 'CM ' features, against the same code fed with already-normalised, already-selected features - the front-end
kernel's own output (1e-6; 2e-6 in f16x3: the bound of tests/test_gpu_extract_batched.py) or the fp64 restatement written to an archive
(5e-5, the oracle bound of the batched tests).  Without the options the driver's output bytes are what they were."""
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import frontend_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "tf_kaldi_speaker_amd")


def rel_err(got, ref):
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / max(np.abs(ref).max(), 1e-30))


def _model(model, pooling="statistics_pooling", precision="f32"):
    """A toy model directory (random weights, moving statistics away from (0, 1)) and a Trainer on it."""
    from tf_kaldi_speaker_amd.model.trainer import Trainer
    from tf_kaldi_speaker_amd.misc.utils import Params
    nnet = os.path.join(model, "nnet")
    os.makedirs(nnet)
    cfg = {"network_type": "tdnn", "loss_func": "softmax", "pooling_type": pooling, "embedding_node": "tdnn6_dense", "seed": 0,
           "last_layer_no_bn": False, "last_layer_linear": False, "weight_l2_regularizer": 1e-2, "batchnorm_momentum": 0.99,
           "optimizer": "sgd", "num_nodes_pooling_layer": 1500, "num_nodes_last_layer": 512, "feature_norm": False, "precision": precision}
    if pooling == "self_attention":
        cfg.update(att_key_num_nodes=[200, 120], att_key_network_type=3, att_use_scale=True, att_key_input="tdnn4_relu",
                   att_value_input="tdnn5_relu", att_num_heads=1, att_split_value=False, att_penalty_term=0.0, att_apply_nonlinear=False)
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
    return tr


def _packed(mats):
    from tf_kaldi_speaker_amd.dataset import kaldi_io
    buf = io.BytesIO()
    for i, m in enumerate(mats):
        kaldi_io.write_compressed_mat(buf, m, key="u%d" % i)
    buf.seek(0)
    out = [m for _, m in kaldi_io.read_mat_ark_packed(buf)]
    assert all(isinstance(m, kaldi_io.PackedMatrix) for m in out)
    return out


@pytest.mark.parametrize("pooling", ["statistics_pooling", "self_attention"], ids=["statistics", "attention"])
@pytest.mark.parametrize("precision", ["f32", "f16x3"])
def test_predict_batch_front_end_equals_its_own_output_fed_back(tmp_path, pooling, precision):
    """(a) raw PackedMatrix items + cmn_window + masks == the front-end kernel's output, read back and passed as host matrices; the same
    for raw host matrices (they take the same kernel) and for VoicedRows pieces that cut chunks out of the kept frames."""
    import torch
    from tf_kaldi_speaker_amd import ops
    from tf_kaldi_speaker_amd.dataset.kaldi_io import VoicedRows
    tr = _model(str(tmp_path / "exp"), pooling, precision)
    rs = np.random.RandomState(13)
    lens = [40, 149, 301, 450, 700, 64]
    items = _packed([R.raw_features(rs, n, 30) for n in lens])
    masks = [(rs.rand(n) < 0.7).astype(np.uint8) for n in lens]
    masks[1][:] = 1
    masks[5][:] = 0
    masks[5][3:60:3] = 1                                   # 19 of 64 frames: above the receptive field (15), far below the raw length
    tol = 1e-6 if precision == "f32" else 2e-6
    got = tr.predict_batch(items, cmn_window=300, voiced=masks)

    def fed_back(first=None, count=None):                  # the kernel's own output for every item, one piece per call
        out = []
        for i, (it, m) in enumerate(zip(items, masks)):
            x = torch.from_numpy(it.decode()[None]).to("cuda:0")
            f = None if first is None else torch.tensor([first[i]], dtype=torch.int32, device="cuda:0")
            c = None if count is None else torch.tensor([count[i]], dtype=torch.int32, device="cuda:0")
            y, rows = ops.frontend(x, torch.tensor([len(m)], dtype=torch.int32, device="cuda:0"), 300, torch.from_numpy(m).to("cuda:0"),
                                   torch.zeros(1, dtype=torch.int64, device="cuda:0"), f, c)
            out.append(y[0, :int(rows[0])].cpu().numpy())
        return out

    ready = fed_back()
    assert [len(r) for r in ready] == [int(m.sum()) for m in masks]
    ref = tr.predict_batch(ready).astype(np.float64)
    assert got.shape == ref.shape == (len(lens), 512)
    plain = tr.predict_batch(items).astype(np.float64)                  # no front end: other features, other embeddings
    assert min(np.abs(ref[i]).max() for i in range(len(lens))) > 1e-3 and rel_err(plain, ref) > 1e-2
    assert rel_err(got, ref) <= tol, rel_err(got, ref)
    host = tr.predict_batch([it.decode() for it in items], cmn_window=300, voiced=masks)
    assert rel_err(host, ref) <= tol, rel_err(host, ref)
    kept = [int(m.sum()) for m in masks]
    first = [k // 3 for k in kept]
    count = [max(15, k // 2) for k in kept]
    count[5] = 15
    first[5] = 2
    assert all(f + c <= k for f, c, k in zip(first, count, kept))
    pieces = [VoicedRows(it, m, f, c) for it, m, f, c in zip(items, masks, first, count)]
    got_p = tr.predict_batch(pieces, cmn_window=300)
    ref_p = tr.predict_batch(fed_back(first, count)).astype(np.float64)
    assert rel_err(got_p, ref_p) <= tol, rel_err(got_p, ref_p)
    with pytest.raises(ValueError, match="receptive field"):           # lengths are post-selection lengths
        short = masks[0].copy()
        short[14:] = 0
        tr.predict_batch(items[:1], cmn_window=300, voiced=[short])
    with pytest.raises(ValueError, match="voicing"):
        tr.predict_batch(items[:1], voiced=[masks[1]])
    tr.close()


def _extract(args, cwd=PKG):
    env = dict(os.environ, TF_KALDI_ROOT=PKG, PYTHONPATH=PKG)
    r = subprocess.run([sys.executable, os.path.join(PKG, "nnet", "lib", "extract.py")] + args, env=env, cwd=cwd, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stderr


def _key_lines(stderr):
    return [ln.split("[INFO] ", 1)[1] for ln in stderr.splitlines() if "[INFO] Key " in ln]


def _summary(stderr):
    ln = [ln for ln in stderr.splitlines() if "[INFO] Extracted " in ln]
    assert len(ln) == 1
    return ln[0].split("[INFO] ", 1)[1].split(" in ")[0]


def test_extract_driver_front_end_equals_prepared_features(tmp_path):
    """(b) extract.py --cmn-window 300 --vad scp: on a raw 'CM ' archive == extract.py on the archive of the fp64 front end's output:
    same keys, order and log lines, embeddings within 5e-5.  One utterance without a VAD entry, one with a mask of the wrong length, one
    unvoiced, one below --min-chunk-size after selection, one above --chunk-size after selection; the VAD comes in another order."""
    from tf_kaldi_speaker_amd.dataset import kaldi_io
    model = str(tmp_path / "exp")
    _model(model).close()
    rs = np.random.RandomState(17)
    lens = {"ok1": 400, "novad": 120, "badlen": 130, "unvoiced": 140, "short": 100, "long": 1000, "ok2": 90}
    raw_ark, ref_ark, vad_ark, vad_scp = (str(tmp_path / n) for n in ("raw.ark", "ref.ark", "vad.ark", "vad.scp"))
    with open(raw_ark, "wb") as f:
        for k, n in lens.items():
            kaldi_io.write_compressed_mat(f, R.raw_features(rs, n, 30), key=k)
    raw = dict(kaldi_io.read_mat_ark(raw_ark))                          # what the decoder gives (the codec is lossy)
    vad = {k: (rs.rand(n) < 0.7).astype(np.float32) for k, n in lens.items()}
    vad["ok2"][:] = 1
    vad["unvoiced"][:] = 0
    vad["short"][:] = 0
    vad["short"][10:90:4] = 1                                            # 20 voiced frames < 25
    vad["badlen"] = vad["badlen"][:-1]
    del vad["novad"]
    assert vad["long"].sum() > 300 and 25 <= vad["ok1"].sum() <= 300
    offsets = {}
    with open(vad_ark, "wb") as f:
        for k in sorted(vad):                                            # not the order of the features
            f.write((k + " ").encode())
            offsets[k] = f.tell()
            kaldi_io.write_vec_flt(f, vad[k])
    with open(vad_scp, "w") as f:
        for k in sorted(vad, reverse=True):
            f.write("%s %s:%d\n" % (k, vad_ark, offsets[k]))
    with open(ref_ark, "wb") as f:
        for k in lens:
            if k in vad and len(vad[k]) == len(raw[k]) and vad[k].any():
                kaldi_io.write_mat(f, R.frontend(raw[k], 300, vad[k]).astype(np.float32), key=k)
    common = ["--chunk-size", "300", "--min-chunk-size", "25", model]
    out_fe, out_ref, out_ark = (str(tmp_path / n) for n in ("fe.ark", "ref_out.ark", "fe_ark.ark"))
    err_fe = _extract(["--cmn-window", "300", "--vad", "scp:" + vad_scp] + common + ["ark:" + raw_ark, "ark:" + out_fe])
    err_ref = _extract(common + ["ark:" + ref_ark, "ark:" + out_ref])
    skips = ["Key novad has no VAD entry, skip.", "Key badlen has 130 frames but 129 VAD decisions, skip.", "Key unvoiced has no voiced frame, skip."]
    lines = _key_lines(err_fe)
    assert [ln for ln in lines if ln in skips] == skips                  # archive order
    assert [ln for ln in lines if ln not in skips] == _key_lines(err_ref)
    assert "Key short length too short, 20 < 25, skip." in lines
    assert "Key long length %d > 300, split to" % int(vad["long"].sum()) in "\n".join(lines)
    assert _summary(err_fe) == _summary(err_ref)                         # utterances and (post-selection) frames
    fe, ref = list(kaldi_io.read_vec_flt_ark(out_fe)), list(kaldi_io.read_vec_flt_ark(out_ref))
    assert [k for k, _ in fe] == [k for k, _ in ref] == ["ok1", "long", "ok2"]
    for (k, a), (_, b) in zip(fe, ref):
        assert rel_err(a, b.astype(np.float64)) <= 5e-5, (k, rel_err(a, b.astype(np.float64)))
    # --vad ark: (read up front) gives the same bytes as --vad scp: (looked up by key)
    _extract(["--cmn-window", "300", "--vad", "ark:" + vad_ark] + common + ["ark:" + raw_ark, "ark:" + out_ark])
    assert open(out_ark, "rb").read() == open(out_fe, "rb").read()


def test_extract_driver_without_the_options_is_unchanged(tmp_path):
    """(c) neither option: two invocations on the mixed archive of tests/test_gpu_extract_batched.py give the same bytes, and both meet that
    test's expectations (keys in archive order, its log lines, each embedding == Trainer.predict one utterance at a time, 1e-6)."""
    from tf_kaldi_speaker_amd.dataset import kaldi_io
    from tf_kaldi_speaker_amd.misc.utils import utterance_embedding
    model = str(tmp_path / "exp")
    tr = _model(model)
    rs = np.random.RandomState(9)
    lens = [90, 20, 410, 33, 150, 149, 151, 25, 700]
    mats = {"utt%02d" % i: (rs.randn(n, 30) * 2).astype(np.float32) for i, n in enumerate(lens)}
    ark_in = str(tmp_path / "in.ark")
    with open(ark_in, "wb") as f:
        for i, (k, m) in enumerate(mats.items()):
            (kaldi_io.write_mat if i % 4 == 3 else kaldi_io.write_compressed_mat)(f, m, key=k)
    feats = dict(kaldi_io.read_mat_ark(ark_in))
    outs = []
    for name in ("out1.ark", "out2.ark"):
        out = str(tmp_path / name)
        err = _extract(["--chunk-size", "300", "--min-chunk-size", "25", model, "ark:" + ark_in, "ark:" + out])
        assert "Key utt01 length too short, 20 < 25, skip." in err and "Key utt02 length 410 > 300, split to 2 segments" in err
        assert not any("VAD" in ln or "voiced" in ln for ln in _key_lines(err))
        outs.append(open(out, "rb").read())
    assert outs[0] == outs[1]
    got = list(kaldi_io.read_vec_flt_ark(str(tmp_path / "out1.ark")))
    assert [k for k, _ in got] == [k for k, m in mats.items() if m.shape[0] >= 25]
    for k, e in got:
        one, _ = utterance_embedding(tr.predict, feats[k], 300, False)
        assert rel_err(e, one.astype(np.float64)) <= 1e-6, (k, rel_err(e, one.astype(np.float64)))
    tr.close()
