"""The engine with the GE2E head (loss kind 6): steps of SGD and Adam against a float64 step composed from the oracle
(oracle/xvector_oracle.py: network forward, backward, regulariser, optimisers) and tests/ge2e_ref.py (the loss, d loss / d embedding, d w and
d b), at the tolerances of tests/test_gpu_engine.py and with the helpers of tests/test_gpu_triplet_engine.py - shrunk widths, 4 speakers x 2
segments, T = 20, both types, with and without feature_norm; one step at 13 x 10 (stage 0's separate launches, more rows than
XV_SEGMENT_MAX_ROWS).  ge2e/w and ge2e/b are compared after every step like every other variable: outside the regulariser, inside the
optimisers.  Decisions keep 64 + 2 x 40 bounds (test_gpu_triplet_engine explains), the seed is chosen when the case is generated.  Then
precision f16x3, with_margin = 0, a repeated step's gradient buffer, the refusals."""
import numpy as np
import pytest
import torch

from oracle import xvector_oracle as O
import ge2e_ref as G
import test_gpu_engine as TE
import test_gpu_triplet_engine as TT

pytestmark = pytest.mark.gpu

D, P, L = TT.D, TT.P, TT.L
W0, B0 = 10.0, -5.0
SCALARS = ("ge2e/w", "ge2e/b")


def start_variables(cfg_o):
    V = TT.start_variables(cfg_o)
    V["ge2e/w"], V["ge2e/b"] = np.float64(W0).reshape(()), np.float64(B0).reshape(())
    return V


def batch(n, m, t, seed):
    """(features [n * m, t, D] float32, labels) speaker-major with a speaker offset"""
    rs = np.random.RandomState(seed)
    x = rs.randn(n * m, t, D) + 0.7 * np.repeat(rs.randn(n, 1, D), m, axis=0)
    return x.astype(np.float32), np.repeat(np.arange(n), m).astype(np.int32)


def oracle_step(V, cfg_o, x, n, m, loss_type, lr, state, eng=None):
    """One float64 step; the ReLU pattern is the GPU's when an engine is given.  The network's variables go through the oracle; the two scalars
    get ge2e_ref's gradients, no regulariser, and the same optimiser."""
    net = {k: v for k, v in V.items() if k not in SCALARS}
    fwd = TE.oracle_forward(net, cfg_o, x.astype(np.float64))
    ep = TE.gpu_relu_pattern(eng, fwd, max_flip_fraction=5e-4, cfg_o=cfg_o) if eng is not None else fwd["ep"]
    res = G.ge2e(fwd["feats"], n, m, float(V["ge2e/w"]), float(V["ge2e/b"]), loss_type)
    grads = O.tdnn_backward(net, cfg_o, ep, fwd["caches"], res.dx)
    reg, Gr = O.regularization(net, cfg_o)
    for k, g in Gr.items():
        grads[k] = grads[k] + g
    grads["ge2e/w"], grads["ge2e/b"] = np.float64(res.dw).reshape(()), np.float64(res.db).reshape(())
    newV, new_state = {}, {"__t__": state.get("__t__", 0) + 1}
    for name, p in V.items():
        if not O.is_trainable(name):
            newV[name] = fwd["bn_new"].get(name, p)
        elif cfg_o.optimizer == "sgd":
            newV[name] = O.sgd_update(p, grads[name].reshape(p.shape), lr)
        else:
            mm, vv = state.get(name, (np.zeros_like(p), np.zeros_like(p)))
            newV[name], mm, vv = O.adam_update(p, grads[name].reshape(p.shape), mm, vv, new_state["__t__"], lr)
            new_state[name] = (mm, vv)
    return newV, new_state, dict(res=res, reg=reg, grads=grads, fwd=fwd)


def stable_seed(cfg_o, n, m, t, loss_type, lr, steps):
    for seed in range(60):
        V, state, gap = start_variables(cfg_o), {}, np.inf
        for it in range(steps):
            x, _ = batch(n, m, t, 1000 * seed + it)
            V, state, info = oracle_step(V, cfg_o, x, n, m, loss_type, lr, state)
            gap = min(gap, info["res"].gap)
        if gap >= 2 * TT.STABLE_ENGINE:
            return seed
    raise AssertionError("no decision-stable case in 60 seeds")


def make_engine(loss_type, cfg_o, n, m, t, V, **kw):
    from tf_kaldi_speaker_amd import engine as E
    c = E.make_config(D, 37, loss_func="ge2e_loss", ge2e_loss_type=loss_type, init_end2end_w=W0, init_end2end_b=B0, num_speakers_per_batch=n,
                      num_segments_per_speaker=m, num_valid_speakers_per_batch=4, num_valid_segments_per_speaker=2, num_nodes_pooling_layer=P,
                      num_nodes_last_layer=L, max_batch=n * m, max_frames=t, optimizer=cfg_o.optimizer, last_layer_linear=True,
                      feature_norm=cfg_o.feature_norm, feature_scaling_factor=1.0, aux_loss_func=("ring_loss",), **kw)
    eng = E.Engine(c)
    assert not [k for k in eng.table if k.startswith("softmax")] and set(eng.table) == set(V)      # no softmax/output/*, no ring radius; w and b
    assert eng.table["ge2e/w"] == ((), eng.table["ge2e/w"][1], True) and eng.table["ge2e/b"][0] == ()
    eng.init_variables(seed=0)
    got = eng.get_variables()
    assert float(got["ge2e/w"]) == W0 and float(got["ge2e/b"]) == B0      # init_end2end_w / _b
    eng.set_variables({k: np.asarray(v, np.float32) for k, v in V.items()})
    return eng


def check_scalars(eng, info):
    """d w and d b: sums of B N terms P c of mixed sign, held as the op-level test holds them - the derived bound, on top of what the
    embedding's own 5e-5 moves them by (as the other gradients' 1e-4 allows)"""
    got, res = eng.get_gradients(), info["res"]
    scale = max(abs(res.dw), abs(res.db))
    assert abs(float(got["ge2e/w"]) - res.dw) <= res.bound_dw + 1e-4 * scale, (float(got["ge2e/w"]), res.dw)
    assert abs(float(got["ge2e/b"]) - res.db) <= res.bound_db + 1e-4 * scale, (float(got["ge2e/b"]), res.db)


class Network(object):
    """the engine without its two scalars, for the helpers of the pairwise heads' test (the scalars are held by check_scalars / check_scalar_update)"""

    def __init__(self, eng):
        self.losses, self.endpoint = eng.losses, eng.endpoint
        self.get_gradients = lambda: {k: v for k, v in eng.get_gradients().items() if k not in SCALARS}
        self.get_variables = lambda: {k: v for k, v in eng.get_variables().items() if k not in SCALARS}


def check_gradients(eng, info, cfg_o):
    TT.check_gradients(Network(eng), dict(info, grads={k: v for k, v in info["grads"].items() if k not in SCALARS}), cfg_o)
    check_scalars(eng, info)


def check_variables(eng, cfg_o, newV, info, lr):
    """the network's variables by the pairwise heads' criterion; w and b after the update: 2e-5 of the value as there, plus what the
    gradient's own allowance (check_scalars) moves an SGD step by.  Adam's step is lr m^ / (sqrt(v^) + 1e-8), at most 2 lr in these first two
    steps whatever the gradient: a gradient that its bound does not tell from 0 - d b of the softmax type, rounding noise around 0 on both
    sides - may send the two sides up to that far apart, any other gives the same step on both."""
    TT.check_variables(Network(eng), cfg_o, {k: v for k, v in newV.items() if k not in SCALARS},
                       dict(info, grads={k: v for k, v in info["grads"].items() if k not in SCALARS}), lr)
    got, res = eng.get_variables(), info["res"]
    scale = max(abs(res.dw), abs(res.db))
    for name, g, bound in (("ge2e/w", res.dw, res.bound_dw), ("ge2e/b", res.db, res.bound_db)):
        tol = 2e-5 * abs(float(newV[name]))
        if cfg_o.optimizer == "sgd":
            tol += lr * (bound + 1e-4 * scale)
        elif abs(g) <= TT.STABLE_ENGINE * bound:
            tol += 2 * lr
        assert abs(float(got[name]) - float(newV[name])) <= tol, (name, float(got[name]), float(newV[name]), tol)


@pytest.mark.parametrize("feature_norm", [False, True], ids=["plain", "feature_norm"])
@pytest.mark.parametrize("optimizer", ["sgd", "adam"])
@pytest.mark.parametrize("loss_type", G.TYPES)
def test_two_steps_match_the_composed_float64_step(loss_type, optimizer, feature_norm):
    n, m, t, lr = 4, 2, 20, (0.05 if optimizer == "sgd" else 0.001)
    cfg_o = TT.oracle_config(optimizer, feature_norm)
    seed = stable_seed(cfg_o, n, m, t, loss_type, lr, 2)
    eng = make_engine(loss_type, cfg_o, n, m, t, start_variables(cfg_o))
    for it in range(2):
        x, lab = batch(n, m, t, 1000 * seed + it)
        V, state = TT.engine_state(eng, cfg_o, it)
        eng.forward(x, True)
        eng.loss(lab, it, True)
        eng.backward(-1)
        newV, _, info = oracle_step(V, cfg_o, x, n, m, loss_type, lr, state, eng)
        assert info["res"].gap >= TT.STABLE_ENGINE, info["res"].gap
        check_gradients(eng, info, cfg_o)
        eng.apply(lr, 1.0)
        check_variables(eng, cfg_o, newV, info, lr)
        after = eng.get_variables()
        assert float(after["ge2e/w"]) != float(V["ge2e/w"]) and (loss_type == G.SOFTMAX or float(after["ge2e/b"]) != float(V["ge2e/b"]))      # they move
    eng.close()


@pytest.mark.parametrize("loss_type", G.TYPES)
def test_one_step_at_13_x_10(loss_type):
    n, m, t, lr = 13, 10, 16, 0.05
    cfg_o = TT.oracle_config("sgd", loss_type == G.SOFTMAX)
    seed = stable_seed(cfg_o, n, m, t, loss_type, lr, 1)
    V = start_variables(cfg_o)
    eng = make_engine(loss_type, cfg_o, n, m, t, V)
    x, lab = batch(n, m, t, 1000 * seed)
    eng.forward(x, True)
    eng.loss(lab, 0, True)
    eng.backward(-1)
    newV, _, info = oracle_step(V, cfg_o, x, n, m, loss_type, lr, {}, eng)
    assert info["res"].gap >= TT.STABLE_ENGINE, info["res"].gap
    check_gradients(eng, info, cfg_o)
    eng.apply(lr, 1.0)
    check_variables(eng, cfg_o, newV, info, lr)
    eng.close()


@pytest.mark.parametrize("loss_type", G.TYPES)
def test_a_repeated_step_gives_the_same_gradient_buffer(loss_type):
    cfg_o = TT.oracle_config("sgd", True)
    eng = make_engine(loss_type, cfg_o, 4, 2, 20, start_variables(cfg_o))
    x, lab = batch(4, 2, 20, 3)
    bufs = []
    for _ in range(2):
        eng.forward(x, True)
        eng.loss(lab, 0, True)
        eng.backward(-1)
        bufs.append(eng.grads.clone())
        eng.grads.zero_()
    assert bufs[0].abs().max() > 0 and torch.equal(bufs[0], bufs[1])
    eng.close()


def test_f16x3_builds_and_steps_with_the_head_in_fp32():
    """the frame layers' contractions in split precision, the embedding and the head in fp32: the head's values are those of the op on the
    engine's own embedding, to the bit"""
    from tf_kaldi_speaker_amd import ops
    cfg_o = TT.oracle_config("sgd", False)
    eng = make_engine(G.SOFTMAX, cfg_o, 4, 2, 20, start_variables(cfg_o), precision="f16x3")
    x, lab = batch(4, 2, 20, 7)
    eng.forward(x, True)
    eng.loss(lab, 0, True)
    eng.backward(-1)
    emb = eng.endpoint("output").contiguous()
    w, b = torch.tensor([W0], device="cuda"), torch.tensor([B0], device="cuda")
    cfg = ops.ge2e_loss_config(G.SOFTMAX, 4, 2)
    loss, _, ws = ops.ge2e_loss(cfg, emb, w, b)
    _, dw, db = ops.ge2e_loss_backward(cfg, emb, w, b, ws)
    g = eng.get_gradients()
    assert np.float32(eng.raw_loss()) == loss.cpu().numpy()[0] and g["ge2e/w"] == dw.cpu().numpy()[0] and g["ge2e/b"] == db.cpu().numpy()[0]
    before = eng.get_variables()
    eng.apply(0.05, 1.0)
    after = eng.get_variables()
    assert all(np.isfinite(v).all() for v in after.values()) and float(after["ge2e/w"]) != float(before["ge2e/w"])
    assert np.abs(after["tdnn/tdnn1_conv/kernel"] - before["tdnn/tdnn1_conv/kernel"]).max() > 0
    eng.close()


def test_without_margin_the_head_gives_the_e2e_validation_value():
    from tf_kaldi_speaker_amd import _lib
    import triplet_ref as R
    cfg_o = TT.oracle_config("sgd", False)
    eng = make_engine(G.CONTRASTIVE, cfg_o, 4, 2, 20, start_variables(cfg_o))
    x, lab = batch(4, 2, 20, 5)
    eng.forward(x, False)
    eng.loss(lab, 0, with_margin=False)
    emb = eng.endpoint("output").cpu().numpy()
    assert abs(eng.raw_loss() - R.e2e_valid_loss(emb, 4, 2)) <= R.e2e_valid_bound(emb, 4, 2)
    eng.forward(x, True)
    eng.loss(lab, 0, with_margin=False)
    with pytest.raises(_lib.XvError, match="end-to-end validation loss, which has no backward"):
        eng.backward(-1)
    eng.forward(x[:6], False)
    with pytest.raises(_lib.XvError, match="4 x 2 rows, the batch has 6"):
        eng.loss(lab[:6], 0, with_margin=False)
    eng.forward(x[:6], True)
    with pytest.raises(_lib.XvError, match="ge2e_loss takes num_speakers_per_batch x num_segments_per_speaker = 4 x 2 rows, the batch has 6"):
        eng.loss(lab[:6], 0, True)
    eng.close()


def test_refusals():
    from tf_kaldi_speaker_amd import _lib, engine as E
    c = E.make_config(D, 0, loss_func="ge2e_loss", num_speakers_per_batch=2, num_segments_per_speaker=2, num_nodes_pooling_layer=P,
                      num_nodes_last_layer=L, max_batch=4, max_frames=20)
    assert c.loss_kind == 6 and c.ge2e_loss.speakers == 2
    opts, c.ge2e_loss = c.ge2e_loss, None
    eng = E.Engine(c)
    x, lab = batch(2, 2, 20, 0)
    eng.forward(x, True)
    with pytest.raises(_lib.XvError, match="\\(ge2e_loss\\) needs its options: call xv_engine_set_ge2e_loss first"):
        eng.loss(lab, 0, True)
    opts.segments = 1
    assert eng.lib.xv_engine_set_ge2e_loss(eng.h, opts) != 0 and b"num_segments_per_speaker is 1" in eng.lib.xv_last_error()
    opts.segments, opts.loss_type = 2, 5
    assert eng.lib.xv_engine_set_ge2e_loss(eng.h, opts) != 0 and b"The GE2E only support softmax and contrastive loss" in eng.lib.xv_last_error()
    eng.close()
    soft = E.Engine(E.make_config(D, 5, num_nodes_pooling_layer=P, num_nodes_last_layer=L, max_batch=4, max_frames=20))
    opts.loss_type = 0
    assert soft.lib.xv_engine_set_ge2e_loss(soft.h, opts) != 0 and b"is not ge2e_loss (6)" in soft.lib.xv_last_error()
    soft.close()
