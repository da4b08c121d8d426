"""Trainer with loss_func "ge2e_loss" on make_data_dir data, both types: an epoch (loss finite, variables and the two scalars moved, no
softmax/output variables), valid(..., batch_type="end2end") returning the value tests/triplet_ref.py gives for the batch it drew, and both
checkpoint formats round-tripping with ge2e/w and ge2e/b to the bit."""
import json
import os

import numpy as np
import pytest

from tests.kaldi_fixture import make_data_dir
import triplet_ref as R
from test_gpu_triplet_trainer import BASE

pytestmark = pytest.mark.gpu

GE2E = dict(loss_func="ge2e_loss", init_end2end_w=10.0, init_end2end_b=-5.0)


@pytest.mark.parametrize("loss_type", ["softmax", "contrastive"])
def test_trainer_trains_validates_and_restores(tmp_path, loss_type):
    from tf_kaldi_speaker_amd.misc.utils import Params
    from tf_kaldi_speaker_amd.model.trainer import Trainer
    data, spklist, _ = make_data_dir(str(tmp_path / "train"), num_spk=6, utts_per_spk=3, min_frames=60, max_frames=90)
    cfg_path = tmp_path / "config.json"
    cfg_path.write_text(json.dumps(dict(BASE, ge2e_loss_type=loss_type, **GE2E)))
    model = str(tmp_path / "exp")
    os.makedirs(os.path.join(model, "nnet"))
    tr = Trainer(Params(str(cfg_path)), model)
    tr.build("train", dim=30, loss_type="ge2e_loss", num_speakers=6)
    tr.build("valid", dim=30, loss_type="ge2e_loss", num_speakers=6)
    assert tr.engine.config.loss_kind == 6 and tr.engine.config.ge2e_loss.loss_type == {"softmax": 0, "contrastive": 1}[loss_type]
    assert not [n for n in tr.engine.table if n.startswith("softmax")]      # no head variables, no softmax_ringloss/r: aux_loss_func is not evaluated
    before = tr.engine.get_variables()
    assert float(before["ge2e/w"]) == 10.0 and float(before["ge2e/b"]) == -5.0
    tr.train(data, spklist, 0.01)
    after = tr.engine.get_variables()
    assert np.isfinite(tr.train_ops["raw_loss"]) and np.isfinite(tr.train_ops["loss"]) and tr.train_ops["raw_loss"] >= 0
    for name in ("tdnn/tdnn1_conv/kernel", "tdnn/tdnn7_dense/kernel", "ge2e/w"):
        assert np.isfinite(after[name]).all() and np.abs(after[name] - before[name]).max() > 0, name
    assert np.isfinite(after["ge2e/b"]) and (loss_type == "softmax" or after["ge2e/b"] != before["ge2e/b"])
    # end2end validation: the value of the batch the loader drew, from the embedding the engine gives for it
    loss, _, _ = tr.valid(data, spklist, batch_type="end2end")
    x, lab = tr._last_valid_features, tr._last_valid_labels
    assert x.shape[0] == 8 and (lab[0::2] == lab[1::2]).all() and np.unique(lab).size == 4      # four speakers in blocks of two
    tr.engine.forward(x, False)
    emb = tr.engine.endpoint("output").cpu().numpy()
    assert abs(loss - R.e2e_valid_loss(emb, 4, 2)) <= R.e2e_valid_bound(emb, 4, 2)
    kept = tr.engine.get_variables()
    assert kept["ge2e/w"] == after["ge2e/w"] and kept["ge2e/b"] == after["ge2e/b"]      # the validation engine's larger batch kept them
    with pytest.raises(AssertionError, match="The batch_type can only be softmax or end2end"):
        tr.valid(data, spklist, batch_type="ge2e")
    tr.close()
    # both checkpoint formats: the .npz, then the TensorFlow payload alone
    prefix = os.path.join(model, "nnet", "model-3")
    assert os.path.isfile(prefix + ".npz") and os.path.isfile(prefix + ".index") and os.path.isfile(prefix + ".data-00000-of-00001")
    for drop_npz in (False, True):
        if drop_npz:
            os.remove(prefix + ".npz")
        tr2 = Trainer(Params(str(cfg_path)), model)
        tr2.build("train", dim=30, loss_type="ge2e_loss", num_speakers=6)
        assert tr2.load() == 3
        got = tr2.engine.get_variables()
        assert set(got) == set(after) and {"ge2e/w", "ge2e/b"} <= set(got)
        for k, v in got.items():
            assert np.array_equal(after[k], v), k
        tr2.close()
