"""The engine with a pairwise loss head (loss kinds 4 / 5): steps of SGD and Adam against a float64 step composed from the oracle
(oracle/xvector_oracle.py: network forward, backward, regulariser, optimisers) and tests/triplet_ref.py (the loss and d loss / d embedding),
at the tolerances of tests/test_gpu_engine.py - shrunk widths, B = 8, T = 20, with and without feature_norm; one step at B = 130 (stage 0's
separate launches, more rows than XV_SEGMENT_MAX_ROWS); with_margin = 0; a repeated step's gradient buffer; the refusals.

The mined decisions must be the same in float64 and on the GPU, whose embedding is itself only held to 5e-5 of the float64 one (the endpoint
tolerance of tests/test_gpu_engine.py, asserted here too): up to 1e-4 in an entry of the pair matrix, some 40 of its rounding bounds, on
either side of a comparison.  A decision is safe at 64 + 2 x 40 bounds from its threshold (STABLE_ENGINE).  The input seed of a case is chosen,
when the case is generated, such that a float64-only simulation of its steps keeps twice that, and the run asserts STABLE_ENGINE on every
step it compares."""
import numpy as np
import pytest
import torch

from oracle import xvector_oracle as O
import test_gpu_engine as TE
import triplet_ref as R

pytestmark = pytest.mark.gpu

D, P, L = 30, 128, 64
STABLE_ENGINE = R.STABLE + 2 * 40.0
HEADS = [("semihard", R.SEMIHARD, dict(margin=0.2, squared=False), dict(loss_func="semihard_triplet_loss", margin=0.2, triplet_loss_squared=False)),
         ("angular-all-am", R.ALL, dict(margin=0.1, margin_kind=2),
          dict(loss_func="angular_triplet_loss", margin=0.1, triplet_type="all", loss_type="additive_margin_softmax")),
         ("angular-hard-arc", R.HARD, dict(margin=0.3, margin_kind=3),
          dict(loss_func="angular_triplet_loss", margin=0.3, triplet_type="hard", loss_type="additive_angular_margin_softmax"))]


def oracle_config(optimizer, feature_norm):
    return O.Config(feat_dim=D, num_speakers=3, num_nodes_pooling_layer=P, num_nodes_last_layer=L, loss_func="softmax", optimizer=optimizer,
                    last_layer_linear=True, feature_norm=feature_norm, feature_scaling_factor=1.0)


def start_variables(cfg_o, seed=0):
    V = O.init_variables(cfg_o, seed=seed, dtype=np.float64)
    rs = np.random.RandomState(seed + 100)
    for k in V:
        if k.endswith(("gamma", "beta", "bias")):
            V[k] = V[k] + 0.1 * rs.randn(*V[k].shape)
    return {k: v.astype(np.float32).astype(np.float64) for k, v in V.items() if not k.startswith("softmax")}


def batch(b, t, seed, copies=1):
    """(features [b, t, D] float32, labels), speaker-major with a speaker offset: b / copies chunks in pairs (13 chunks: groups of 3, 4 and 6);
    copies > 1: the chunks repeated under labels of their own"""
    rs = np.random.RandomState(seed)
    n = b // copies
    sizes = [3, 4, 6] if n == 13 else [2] * (n // 2)
    lab = np.repeat(np.arange(len(sizes)), sizes)
    x = rs.randn(n, t, D) + 0.7 * np.repeat(rs.randn(len(sizes), 1, D), sizes, axis=0)
    x, lab = np.tile(x, (copies, 1, 1)), np.concatenate([lab + len(sizes) * c for c in range(copies)])
    return x.astype(np.float32), lab.astype(np.int32)


def oracle_step(V, cfg_o, x, labels, kind, opt, lr, state, eng=None):
    """One float64 step; the ReLU pattern is the GPU's when an engine is given (test_gpu_engine.oracle_step_with_gpu_relu_pattern)"""
    fwd = TE.oracle_forward(V, cfg_o, x.astype(np.float64))
    # (max_flip_fraction: the pooled layer has 8 x 6 x 128 = 6144 outputs at these widths, ONE rounding-level flip is 1.6e-4 of them; the bound on
    # the pre-activation of a flipped unit, 2e-5 of the layer's scale, is the helper's own)
    ep = TE.gpu_relu_pattern(eng, fwd, max_flip_fraction=5e-4, cfg_o=cfg_o) if eng is not None else fwd["ep"]
    res = R.pair_loss(fwd["feats"], labels, kind, **opt)
    G = O.tdnn_backward(V, cfg_o, ep, fwd["caches"], res.dx)
    reg, Gr = O.regularization(V, cfg_o)
    for k, g in Gr.items():
        G[k] = G[k] + g
    newV, new_state = {}, {"__t__": state.get("__t__", 0) + 1}
    for name, p in V.items():
        if not O.is_trainable(name):
            newV[name] = fwd["bn_new"].get(name, p)
        elif cfg_o.optimizer == "sgd":
            newV[name] = O.sgd_update(p, G[name].reshape(p.shape), lr)
        else:
            m, v = state.get(name, (np.zeros_like(p), np.zeros_like(p)))
            newV[name], m, v = O.adam_update(p, G[name].reshape(p.shape), m, v, new_state["__t__"], lr)
            new_state[name] = (m, v)
    return newV, new_state, dict(res=res, reg=reg, grads=G, fwd=fwd)


def stable_seed(cfg_o, b, t, kind, opt, lr, steps, copies=1):
    for seed in range(60):
        V, state, gap = start_variables(cfg_o), {}, np.inf
        for it in range(steps):
            x, lab = batch(b, t, 1000 * seed + it, copies)
            V, state, info = oracle_step(V, cfg_o, x, lab, kind, opt, lr, state)
            gap = min(gap, info["res"].gap)
        if gap >= 2 * STABLE_ENGINE:
            return seed
    raise AssertionError("no decision-stable case in 60 seeds")


def make_engine(ekw, cfg_o, b, t, V):
    from tf_kaldi_speaker_amd import engine as E
    c = E.make_config(D, 37, num_nodes_pooling_layer=P, num_nodes_last_layer=L, max_batch=b, max_frames=t, optimizer=cfg_o.optimizer,
                      last_layer_linear=True, feature_norm=cfg_o.feature_norm, feature_scaling_factor=1.0, num_valid_speakers_per_batch=4,
                      num_valid_segments_per_speaker=2, **ekw)
    eng = E.Engine(c)
    assert not [n for n in eng.table if n.startswith("softmax")] and set(eng.table) == set(V)      # no softmax/output/* whatever num_speakers says
    eng.set_variables({k: v.astype(np.float32) for k, v in V.items()})
    return eng


def check_gradients(eng, info, cfg_o):
    raw, reg = eng.losses()
    res = info["res"]
    assert abs(raw - res.loss) <= 2e-5 * abs(res.loss) + 1e-6, (raw, res.loss)
    assert abs(reg - info["reg"]) <= 2e-5 * abs(info["reg"])
    assert TE.rel_err(eng.endpoint("output").cpu().numpy(), info["fwd"]["ep"]["output"]) <= 5e-5
    for name, g in eng.get_gradients().items():
        ref = info["grads"][name].reshape(g.shape)
        if name.endswith("_conv/bias") or name.endswith("_dense/bias"):      # in front of a BatchNorm (tdnn7 too: last_layer_no_bn is off): exactly 0 + noise
            assert np.abs(g).max() <= 1e-4 * max(1.0, np.abs(info["grads"][name.replace("/bias", "/kernel")]).max()), name
            continue
        if name == "tdnn/tdnn7_bn/beta" and np.abs(ref).max() <= 1e-12 * np.abs(info["grads"]["tdnn/tdnn7_dense/kernel"]).max():
            # Euclidean distances do not move with a shift of every embedding: without l2_scaling behind it this gradient is exactly 0, noise on both sides
            assert np.abs(g).max() <= 1e-4 * np.abs(info["grads"]["tdnn/tdnn7_dense/kernel"]).max(), name
            continue
        assert np.isfinite(g).all() and TE.rel_err(g, ref) <= 1e-4, (name, TE.rel_err(g, ref))


def engine_state(eng, cfg_o, steps_done):
    """(variables, optimiser state) of the engine as the float64 step takes them: each step is compared from the engine's own state, since
    Adam's first steps are lr * sign(g) and a gradient entry of rounding size sends two trajectories 2 lr apart in that entry"""
    V = TE.OrderedDictF64(eng.get_variables())
    state = {"__t__": steps_done}
    if cfg_o.optimizer == "adam" and steps_done:
        flat = eng.opt_state.cpu().numpy().astype(np.float64)
        for name, (shape, off, trainable) in eng.table.items():
            if trainable:
                n = int(np.prod(shape)) if len(shape) else 1
                state[name] = (flat[off:off + n].reshape(V[name].shape), flat[eng.n_train + off:eng.n_train + off + n].reshape(V[name].shape))
    return V, state


def check_variables(eng, cfg_o, newV, info, lr):
    """after eng.apply: test_gpu_engine.compare_step_with_oracle's criterion for the variables"""
    for name, v in eng.get_variables().items():
        if name.endswith("/bias"):
            continue
        ref = newV[name]
        diff, slack = np.abs(v - ref), 0.0
        if name in info["grads"]:
            gref = np.abs(info["grads"][name].reshape(v.shape))
            if name == "tdnn/tdnn7_bn/beta" and gref.max() <= 1e-12 * np.abs(info["grads"]["tdnn/tdnn7_dense/kernel"]).max():
                continue      # exactly 0 in float64 (check_gradients): Adam steps lr * sign(noise)
            if cfg_o.optimizer == "adam":
                diff = diff[gref >= 1e-3 * gref.max()]
            else:
                slack = lr * 1e-4 * gref.max()
        assert diff.max() <= 2e-5 * max(np.abs(ref).max(), 1e-12) + slack, (name, diff.max())


@pytest.mark.parametrize("feature_norm", [False, True], ids=["plain", "feature_norm"])
@pytest.mark.parametrize("optimizer", ["sgd", "adam"])
@pytest.mark.parametrize("name,kind,opt,ekw", HEADS, ids=[h[0] for h in HEADS])
def test_two_steps_match_the_composed_float64_step(name, kind, opt, ekw, optimizer, feature_norm):
    b, t, lr = 8, 20, (0.05 if optimizer == "sgd" else 0.001)
    cfg_o = oracle_config(optimizer, feature_norm)
    seed = stable_seed(cfg_o, b, t, kind, opt, lr, 2)
    eng = make_engine(ekw, cfg_o, b, t, start_variables(cfg_o))
    for it in range(2):
        x, lab = batch(b, t, 1000 * seed + it)
        V, state = engine_state(eng, cfg_o, it)
        eng.forward(x, True)
        eng.loss(lab, it, True)
        eng.backward(-1)
        newV, _, info = oracle_step(V, cfg_o, x, lab, kind, opt, lr, state, eng)
        assert info["res"].gap >= STABLE_ENGINE, info["res"].gap
        check_gradients(eng, info, cfg_o)
        eng.apply(lr, 1.0)
        check_variables(eng, cfg_o, newV, info, lr)
    eng.close()


@pytest.mark.parametrize("name,kind,opt,ekw", HEADS, ids=[h[0] for h in HEADS])
def test_a_repeated_step_gives_the_same_gradient_buffer(name, kind, opt, ekw):
    cfg_o = oracle_config("sgd", True)
    eng = make_engine(ekw, cfg_o, 8, 20, start_variables(cfg_o))
    x, lab = batch(8, 20, 3)
    bufs = []
    for _ in range(2):
        eng.forward(x, True)
        eng.loss(lab, 0, True)
        eng.backward(-1)
        bufs.append(eng.grads.clone())
        eng.grads.zero_()
    assert bufs[0].abs().max() > 0 and torch.equal(bufs[0], bufs[1])
    eng.close()


@pytest.mark.parametrize("name,kind,opt,ekw", HEADS, ids=[h[0] for h in HEADS])
def test_one_step_at_130_rows(name, kind, opt, ekw):
    """13 chunks ten times over under labels of their own (tests/triplet_ref.py: sized_case explains why): stage 0 runs its separate launches"""
    b, t, lr = 130, 16, 0.05
    cfg_o = oracle_config("sgd", kind == R.SEMIHARD)
    seed = stable_seed(cfg_o, b, t, kind, opt, lr, 1, copies=10)
    V = start_variables(cfg_o)
    eng = make_engine(ekw, cfg_o, b, t, V)
    x, lab = batch(b, t, 1000 * seed, copies=10)
    eng.forward(x, True)
    eng.loss(lab, 0, True)
    eng.backward(-1)
    out = eng.endpoint("output").cpu().numpy()
    assert all((out[13 * c:13 * c + 13] == out[:13]).all() for c in range(10)), "equal chunks must give equal embeddings for the ties to fall alike"
    newV, _, info = oracle_step(V, cfg_o, x, lab, kind, opt, lr, {}, eng)
    assert info["res"].gap >= STABLE_ENGINE, info["res"].gap
    check_gradients(eng, info, cfg_o)
    eng.close()


def test_without_margin_the_angular_kind_gives_the_e2e_value_and_the_semihard_kind_its_own():
    from tf_kaldi_speaker_amd import _lib
    cfg_o = oracle_config("sgd", False)
    V = start_variables(cfg_o)
    x, lab = batch(8, 20, 5)
    for name, kind, opt, ekw in HEADS[:2]:
        eng = make_engine(ekw, cfg_o, 8, 20, V)
        eng.forward(x, False)
        eng.loss(lab, 0, with_margin=False)
        emb = eng.endpoint("output").cpu().numpy()
        got = eng.raw_loss()
        if kind == R.SEMIHARD:
            ref = R.pair_loss(emb, lab, kind, backward=False, **opt)
            assert abs(got - ref.loss) <= ref.bound
        else:
            assert abs(got - R.e2e_valid_loss(emb, 4, 2)) <= R.e2e_valid_bound(emb, 4, 2)
            eng.forward(x, True)
            eng.loss(lab, 0, with_margin=False)
            with pytest.raises(_lib.XvError, match="end-to-end validation loss, which has no backward"):
                eng.backward(-1)
            eng.forward(x[:6], False)
            with pytest.raises(_lib.XvError, match="4 x 2 rows, the batch has 6"):
                eng.loss(lab[:6], 0, with_margin=False)
        eng.close()


def test_refusals():
    from tf_kaldi_speaker_amd import _lib, engine as E
    c = E.make_config(D, 0, loss_func="angular_triplet_loss", margin=0.1, num_nodes_pooling_layer=P, num_nodes_last_layer=L, max_batch=4, max_frames=20)
    assert c.loss_kind == 5 and c.pair_loss.kind == 1
    opts, c.pair_loss = c.pair_loss, None
    eng = E.Engine(c)
    x, lab = batch(4, 20, 0)
    eng.forward(x, True)
    with pytest.raises(_lib.XvError, match="angular_triplet_loss\\) needs its options: call xv_engine_set_pair_loss first"):
        eng.loss(lab, 0, True)
    opts.kind = 0
    assert eng.lib.xv_engine_set_pair_loss(eng.h, opts) != 0 and b"does not belong to the engine's loss_kind 5" in eng.lib.xv_last_error()
    eng.close()
    soft = E.Engine(E.make_config(D, 5, num_nodes_pooling_layer=P, num_nodes_last_layer=L, max_batch=4, max_frames=20))
    opts.kind = 1
    assert soft.lib.xv_engine_set_pair_loss(soft.h, opts) != 0 and b"is not a pairwise head" in soft.lib.xv_last_error()
    soft.close()
