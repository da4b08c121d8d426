"""The GE2E training loss on the CPU: tests/ge2e_ref.py against the values the reference's own NumPy statement gave
(tests/golden/ge2e_golden.npz, written by tests/golden/make_ge2e_golden.py) within ge2e_ref.oracle_eps_bound, its route through u = X^ X^T
against the TensorFlow body on the rows, its backward against central differences of that body, the decision-stable cases the GPU tests
use, and the host layer: the kinds record, make_config, the refusals with their texts, the initial values of w and b."""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import ge2e_ref as G  # noqa: E402
import make_ge2e_golden as M  # noqa: E402
import triplet_ref as R  # noqa: E402

GOLDEN = np.load(os.path.join(HERE, "golden", "ge2e_golden.npz"))
CASES = sorted(set(k.split("/")[0] for k in GOLDEN.files))


def test_golden_holds_every_case_type_and_scale():
    assert len(CASES) == 7 and sum(c.startswith("hostile") for c in CASES) == 1
    for c in CASES:
        for t in G.TYPES:
            for w, b in G.WB:
                assert M.ge2e_key(c, t, w, b) in GOLDEN.files
    assert G.WB == ((10.0, -5.0), (20.0, 0.0), (1.0, 0.5))


@pytest.mark.parametrize("case", CASES)
def test_restatement_matches_the_reference_oracle(case):
    """No hand-picked constant: the oracle's epsilons bound the difference.  Largest ratios over the golden file: 0.999997 (hostile rows) and
    0.995, both the softmax type at w = 20, where the log's 1e-16 over a small target probability is the whole difference and log(1 + x) <= x
    keeps it below the bound."""
    x = GOLDEN[case + "/x"]
    n, m, _ = GOLDEN[case + "/shape"]
    for t in G.TYPES:
        for w, b in G.WB:
            res = G.ge2e(x, n, m, w, b, t, backward=False)
            want, bound = float(GOLDEN[M.ge2e_key(case, t, w, b)]), G.oracle_eps_bound(x, n, m, w, b, t)
            print("%s %s w=%g b=%g: %.12g oracle %.12g difference %.3g bound %.3g ratio %.3f" % (case, t, w, b, res.loss, want, abs(res.loss - want), bound,
                                                                                             abs(res.loss - want) / bound))
            assert abs(res.loss - want) <= bound
            # the route through u against the TensorFlow body on the rows, in float64: the roundings of D products and 2 M rows per cosine
            assert abs(G.direct(x, n, m, w, b, t) - res.loss) <= (x.shape[1] + 2 * m + 16) * G.U64 * (abs(w) + abs(b) + 1)
            if not case.startswith("hostile"):
                assert res.gap >= G.STABLE
                ev32 = G.ge2e(x, n, m, w, b, t, backward=False, dt=np.float32)
                assert abs(ev32.loss - res.loss) <= res.bound and abs(ev32.dw - res.dw) <= res.bound_dw and abs(ev32.db - res.db) <= res.bound_db


def test_softmax_type_is_the_validation_loss_at_w_20_b_0():
    for case in CASES:
        x = GOLDEN[case + "/x"]
        n, m, _ = GOLDEN[case + "/shape"]
        assert abs(G.ge2e(x, n, m, 20.0, 0.0, G.SOFTMAX, backward=False).loss - R.e2e_valid_loss(x, n, m)) <= 64 * G.U64 * 20


def central(x, n, m, w, b, t, h=1e-6):
    x = R.f64(x)
    num = np.zeros_like(x)
    for i in range(x.shape[0]):
        for j in range(x.shape[1]):
            xp, xm = x.copy(), x.copy()
            xp[i, j] += h
            xm[i, j] -= h
            num[i, j] = (G.direct(xp, n, m, w, b, t) - G.direct(xm, n, m, w, b, t)) / (2 * h)
    dw = (G.direct(x, n, m, w + h, b, t) - G.direct(x, n, m, w - h, b, t)) / (2 * h)
    db = (G.direct(x, n, m, w, b + h, t) - G.direct(x, n, m, w, b - h, t)) / (2 * h)
    return num, dw, db


def difference_tolerance(loss, scale, w, h=1e-6):
    """of a central difference with step h: the two values round at 2^-53 of the loss and of the logits (|w| + 1) each, over 2 h (four to
    spare), and h^2 / 6 times a third derivative, which a smooth function of |w| cosines has within (|w| + 1)^3 of the first's scale"""
    return 8 * G.U64 * (abs(loss) + abs(w) + 1) / (2 * h) + h * h / 6 * (abs(w) + 1) ** 3 * scale


@pytest.mark.parametrize("loss_type", G.TYPES)
@pytest.mark.parametrize("n,m,dim", [(4, 3, 8), (1, 2, 8), (3, 2, 8), (2, 2, 4)])
@pytest.mark.parametrize("w,b", [(10.0, -5.0), (-3.0, 0.5), (1.0, 0.5)])
def test_backward_matches_central_differences(loss_type, n, m, dim, w, b):
    """On a decision-stable case (gap 256 bounds of some 1e-6 against a step of 1e-6) the loss is smooth within the step; negative w is held
    here and by the restatement only (the oracle has w, not |w|)."""
    _, x = G.sized_case(n, m, dim, loss_type, w, b, factor=4)
    res = G.ge2e(R.f64(x), n, m, w, b, loss_type)
    num, dw, db = central(x, n, m, w, b, loss_type)
    tol = difference_tolerance(res.loss, max(np.abs(res.dx).max(), abs(res.dw), abs(res.db)), w)
    assert np.abs(num - res.dx).max() <= tol and abs(dw - res.dw) <= tol and abs(db - res.db) <= tol
    if n > 1:
        assert np.abs(res.dx).max() > 0


@pytest.mark.parametrize("loss_type", G.TYPES)
def test_w_zero_has_no_gradient_but_d_b(loss_type):
    _, x = G.sized_case(3, 2, 8, loss_type)
    res = G.ge2e(R.f64(x), 3, 2, 0.0, 0.5, loss_type)
    num, _, db = central(x, 3, 2, 0.0, 0.5, loss_type)
    tol = difference_tolerance(res.loss, abs(res.db), 0.0)
    assert res.dw == 0 and np.abs(res.dx).max() == 0 and np.abs(num).max() <= tol and abs(db - res.db) <= tol      # sign(0) = 0, as tf.abs has it


@pytest.mark.parametrize("name", sorted(G.hostile_cases()))
@pytest.mark.parametrize("loss_type", G.TYPES)
def test_hostile_cases_are_decision_stable_and_differentiable_off_the_clamps(name, loss_type):
    """Every clamp of a hostile case is decision-stable against 1e-12 (or exactly 0 in any arithmetic), and where no clamp and no tie is active -
    the rows of the speakers that hold no hostile row, and w, b - the backward is the central difference."""
    x, w, b = G.hostile_cases()[name]
    res = G.ge2e(R.f64(x), 4, 2, w, b, loss_type)
    assert res.gap >= G.STABLE and np.isfinite(res.dx).all() and np.isfinite([res.loss, res.dw, res.db]).all()
    if name in ("zero row", "x and -x", "w = 0"):      # the clamped norm, and |w| at 0, have a kink here: held by the stated rules, not by differences
        return
    num, dw, db = central(x, 4, 2, w, b, loss_type)
    tol = difference_tolerance(res.loss, max(np.abs(res.dx).max(), abs(res.dw), abs(res.db)), w)
    assert np.abs(num - res.dx).max() <= tol and abs(dw - res.dw) <= tol and abs(db - res.db) <= tol


def test_clamped_centre_passes_no_gradient_through_its_norm():
    """x and -x: the centre's norm is clamped and the numerator keeps rsqrt(1e-12): a row of another speaker feels the centre's rows through
    |w| P 1e6 x^, the stated rule, and the loss does not move with the clamped norm"""
    x, w, b = G.hostile_cases()["x and -x"]
    res = G.ge2e(R.f64(x), 4, 2, w, b, G.SOFTMAX)
    assert res.nk[1] == 0 and (res.c[[0, 1, 4, 5, 6, 7], 1] == 0).all() and np.abs(res.dx[2:4]).max() > 1e2


@pytest.mark.parametrize("n,m,dim,pitch,types", G.SHAPES)
def test_listed_cases_are_decision_stable(n, m, dim, pitch, types):
    """stable_case finds every listed seed within its 200 tries (the contrastive maximum over N - 1 candidates per row is the decision)"""
    for t in types:
        seed, x = G.sized_case(n, m, dim, t)
        res = G.ge2e(x, n, m, G.OP_W, G.OP_B, t, backward=False)
        assert seed < 200 and res.gap >= G.STABLE and x.dtype == np.float32 and x.shape == (n * m, dim)
    assert (G.CONTRASTIVE in types) == (n * m <= 130)


# ------------------------------------------------------------------ host layer
def test_kinds_record():
    from tf_kaldi_speaker_amd import _lib, kinds
    k = kinds.loss("ge2e_loss")
    assert k.family == kinds.GE2E and k.code == 6 == _lib.LOSS_KINDS["ge2e_loss"] and k.pair_code is None
    assert [n for n, r in kinds.LOSSES.items() if r.family == kinds.GE2E] == ["ge2e_loss"]
    d = dict(ge2e_loss_type="contrastive", init_end2end_w=10, init_end2end_b=-5, num_speakers_per_batch=64, num_segments_per_speaker=10,
             num_valid_speakers_per_batch=8, num_valid_segments_per_speaker=4)
    assert k.keywords(d) == dict(ge2e_loss_type="contrastive", init_end2end_w=10.0, init_end2end_b=-5.0, num_speakers_per_batch=64,
                                 num_segments_per_speaker=10, num_valid_speakers_per_batch=8, num_valid_segments_per_speaker=4, aux_loss_func=())
    with pytest.raises(AssertionError):
        k.keywords(dict(d, num_segments_per_speaker=1))
    with pytest.raises(ValueError, match="^The GE2E only support softmax and contrastive loss$"):
        k.keywords(dict(d, ge2e_loss_type="hinge"))
    with pytest.raises(NotImplementedError, match="Not implement generalized_angular_triplet_loss loss"):
        kinds.loss("generalized_angular_triplet_loss")


def test_make_config_of_the_ge2e_kind():
    """Fails without the feature: make_config(30, 0, loss_func="ge2e_loss") raises NotImplementedError("Not implement ge2e_loss loss")."""
    from tf_kaldi_speaker_amd import _lib, engine as E
    c = E.make_config(30, 0, loss_func="ge2e_loss")
    assert c.loss_kind == 6 and c.pair_loss is None and c.ge2e_init == {"ge2e/w": 10.0, "ge2e/b": -5.0}
    c = E.make_config(30, 7351, loss_func="ge2e_loss", ge2e_loss_type="contrastive", init_end2end_w=20, init_end2end_b=-1.5, num_speakers_per_batch=64,
                      num_segments_per_speaker=10, num_valid_speakers_per_batch=8, num_valid_segments_per_speaker=4, aux_loss_func=("ring_loss",))
    g = c.ge2e_loss
    assert (g.loss_type, g.speakers, g.segments, g.valid_speakers, g.valid_segments) == (1, 64, 10, 8, 4) and c.aux_ring == 0
    assert g.struct_bytes == ctypes.sizeof(_lib.XvGe2eConfig) == 24 and c.ge2e_init == {"ge2e/w": 20.0, "ge2e/b": -1.5}
    assert E.make_config(30, 10).ge2e_loss is None and E.make_config(30, 0, loss_func="semihard_triplet_loss").ge2e_loss is None
    assert _lib.ABI_VERSION == 3 and ctypes.sizeof(_lib.XvConfig) == 268 and ctypes.sizeof(_lib.XvPairLossConfig) == 32      # the layouts stay
    with pytest.raises(AssertionError):
        E.make_config(30, 0, loss_func="ge2e_loss", num_speakers_per_batch=8, num_segments_per_speaker=1)
    with pytest.raises(ValueError, match="^The GE2E only support softmax and contrastive loss$"):
        E.make_config(30, 0, loss_func="ge2e_loss", ge2e_loss_type="triplet", num_speakers_per_batch=8, num_segments_per_speaker=2)
    for name in ("xv_ge2e_loss_workspace_bytes", "xv_ge2e_loss_forward", "xv_ge2e_loss_backward", "xv_engine_set_ge2e_loss"):
        assert name in _lib.SIGNATURES


def test_trainer_build_accepts_the_kind_up_to_the_device():
    """Fails without the feature: Trainer.build(..., loss_type="ge2e_loss") raises NotImplementedError before it looks for a device.  With it,
    build gets as far as the engine: on a box without a GPU that is XvError("No HIP device visible ..."), with one the engine of kind 6."""
    import json
    import tempfile
    from tf_kaldi_speaker_amd import _lib
    from tf_kaldi_speaker_amd.misc.utils import Params
    from tf_kaldi_speaker_amd.model.trainer import Trainer
    conf = dict(seed=0, network_type="tdnn", last_layer_no_bn=False, last_layer_linear=True, feature_norm=False, pooling_type="statistics_pooling",
                num_nodes_pooling_layer=64, num_nodes_last_layer=32, weight_l2_regularizer=1e-2, batchnorm_momentum=0.99, clip_gradient=False,
                num_speakers_per_batch=3, num_segments_per_speaker=2, num_valid_speakers_per_batch=2, num_valid_segments_per_speaker=2,
                max_segment_len=40, ge2e_loss_type="softmax", init_end2end_w=10.0, init_end2end_b=-5.0)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "config.json")
        with open(path, "w") as f:
            json.dump(conf, f)
        tr = Trainer(Params(path), tmp)
        try:
            tr.build("train", dim=30, loss_type="ge2e_loss", num_speakers=6)
        except _lib.XvError as e:
            assert "No HIP device visible" in str(e)
        else:
            assert tr.engine.config.loss_kind == 6 and "ge2e/w" in tr.engine.table
            tr.close()
        assert tr.loss_network.__name__ == "ge2e_loss"


def test_refusals_by_name():
    import torch
    from tf_kaldi_speaker_amd import ops
    cfg = ops.ge2e_loss_config("softmax", 4, 2)
    w = b = torch.zeros(1)
    with pytest.raises(AssertionError):
        ops.ge2e_loss_config("softmax", 8, 1)
    with pytest.raises(ValueError, match="^The GE2E only support softmax and contrastive loss$"):
        ops.ge2e_loss_config("hard", 4, 2)
    bad = ops.ge2e_loss_config("softmax", 8, 2)
    bad.segments = 1
    with pytest.raises(ValueError, match="^ge2e loss: num_segments_per_speaker is 1: a row needs another row of its speaker$"):
        ops.ge2e_loss(bad, torch.zeros(8, 8), w, b)
    with pytest.raises(ValueError, match="^ge2e loss: 6 rows are not 4 speakers x 2 segments$"):
        ops.ge2e_loss(cfg, torch.zeros(6, 8), w, b)
    with pytest.raises(ValueError, match="^ge2e loss: 1026 rows, 2 .. 1024 are supported$"):
        ops.ge2e_loss(ops.ge2e_loss_config("softmax", 513, 2), torch.zeros(1026, 8), w, b)
    with pytest.raises(ValueError, match=r"^ge2e loss: the embedding dimension 6 must be a positive multiple of 4 \(x has 6 columns\)$"):
        ops.ge2e_loss(cfg, torch.zeros(8, 6), w, b)
    with pytest.raises(ValueError, match="^ge2e loss: w must be 1 contiguous float32 values$"):
        ops.ge2e_loss(cfg, torch.zeros(8, 8), torch.zeros(2), b)
    with pytest.raises(ValueError, match="^ge2e loss: the backward needs the workspace ge2e_loss returned for the same cfg, x, w and b$"):
        ops.ge2e_loss_backward(cfg, torch.zeros(8, 8), w, b, None)


def test_initial_values_of_w_and_b():
    from tf_kaldi_speaker_amd import kinds
    rs = np.random.RandomState(0)
    assert kinds.initial_value("w", (), rs, 10.0) == np.float32(10.0) and kinds.initial_value("b", (), rs, -5.0).dtype == np.float32
    assert kinds.initial_value("b", (1,), rs, -5.0).tolist() == [-5.0]


def test_struct_layout_matches_the_header():
    import test_abi
    from tf_kaldi_speaker_amd import _lib
    test_abi.check_struct(test_abi.HEADER, "xv_ge2e_config", _lib.XvGe2eConfig)
    assert _lib.GE2E_TYPES == {"softmax": 0, "contrastive": 1}
