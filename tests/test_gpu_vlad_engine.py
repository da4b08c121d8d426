"""The engine with pooling_type ghost_vlad against a float64 whole-step reference composed from the oracle and tests/vlad_ref.py.

oracle/xvector_oracle.py knows statistics and attention pooling.  Its tdnn_forward / tdnn_backward call statistics_pooling_fwd / _bwd by their
module names, so for these tests the two names are bound to vlad_ref's forward / backward on the step's VLAD variables, tdnn_backward also
returns the VLAD parameter gradients and regularization also covers the centres (pooling.py:256; the assignment kernel is a "/kernel" and is
covered already).  Everything else - the helpers that take the GPU's ReLU pattern, the comparison of the loss, every endpoint, every
gradient, the updated variables and the moving statistics - is tests/test_gpu_engine.py's, at its tolerances; inference through
forward_lengths at those of tests/test_gpu_extract_batched.py."""
import numpy as np
import pytest

import test_gpu_engine as TE
import vlad_ref as V
from oracle import xvector_oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture
def vlad_oracle(monkeypatch):
    """-> state dict; set state["V"] (the step's variables), state["k"] and state["final"] before an oracle call."""
    state = {}

    def names():
        return "tdnn/vlad/vlad_weight_affine/kernel", "tdnn/vlad/vlad_weight_affine/bias", "tdnn/vlad/vlad_centers"

    def pool_fwd(h):
        w, b, c = (state["V"][n] for n in names())
        return V.vlad_forward(h, w, b, c, state["k"], state["final"])

    def pool_bwd(x, cache, dout):
        dx, dw, db, dc = V.vlad_backward(dout, cache, l2=0.0)
        state["G"] = dict(zip(names(), (dw, db, dc)))
        return dx

    tdnn_backward, regularization = O.tdnn_backward, O.regularization

    def backward(Vv, cfg, ep, caches, dout):
        G = tdnn_backward(Vv, cfg, ep, caches, dout)
        G.update(state.pop("G"))
        return G

    def reg(Vv, cfg):
        total, G = regularization(Vv, cfg)
        c = Vv[names()[2]]
        G[names()[2]] = cfg.weight_l2_regularizer * c
        return total + O.l2_regularizer(c, cfg.weight_l2_regularizer), G

    monkeypatch.setattr(O, "statistics_pooling_fwd", pool_fwd)
    monkeypatch.setattr(O, "statistics_pooling_bwd", pool_bwd)
    monkeypatch.setattr(O, "tdnn_backward", backward)
    monkeypatch.setattr(O, "regularization", reg)
    return state


def make(kw, B, T, P, K, G, final, N=37, L=64, seed=0):
    """Engine + oracle config + float64 variables that start from the engine's exact float32 values (every group off its trivial
    initial value, as test_gpu_engine._make)."""
    from tf_kaldi_speaker_amd import engine as E
    cfg_o = O.Config(feat_dim=30, num_speakers=N, num_nodes_pooling_layer=P, num_nodes_last_layer=L, **kw)
    ekw = dict(kw)
    ekw.pop("loss_func", None)
    eng = E.Engine(E.make_config(30, N, loss_func=kw.get("loss_func", "softmax"), num_nodes_pooling_layer=P, num_nodes_last_layer=L, max_batch=B,
                                 max_frames=T, pooling_type="ghost_vlad", vlad_num_centers=K, vlad_num_ghosts=G, vlad_final_l2_norm=final,
                                 precision="f32", **ekw))
    eng.init_variables(seed=seed)
    Vv = eng.get_variables()
    rs = np.random.RandomState(seed + 100)
    for k in Vv:
        if k.endswith(("gamma", "beta", "bias")):
            Vv[k] = Vv[k] + 0.1 * rs.randn(*Vv[k].shape)
        if k.endswith("moving_mean"):
            Vv[k] = 0.2 * rs.randn(*Vv[k].shape)
        if k.endswith("moving_variance"):
            Vv[k] = 0.5 + rs.rand(*Vv[k].shape)
    eng.set_variables({k: v.astype(np.float32) for k, v in Vv.items()})
    return eng, cfg_o, TE.OrderedDictF64(eng.get_variables())


def test_variable_table_and_arena():
    from tf_kaldi_speaker_amd import engine as E
    eng, _, Vv = make(dict(loss_func="softmax"), 4, 30, 48, 3, 2, False)
    names = list(eng.table)
    i = names.index("tdnn/vlad/vlad_weight_affine/kernel")
    assert names[i:i + 3] == ["tdnn/vlad/vlad_weight_affine/kernel", "tdnn/vlad/vlad_weight_affine/bias", "tdnn/vlad/vlad_centers"]
    assert names[i - 1].startswith("tdnn/tdnn5_bn/") and names[i + 3] == "tdnn/tdnn6_dense/kernel"      # where the attention variables sit
    assert eng.table["tdnn/vlad/vlad_weight_affine/kernel"][0] == (48, 5) and eng.table["tdnn/vlad/vlad_centers"][0] == (5, 48)
    assert eng.table["tdnn/tdnn6_dense/kernel"][0] == (3 * 48, 512) and all(eng.table[n][2] for n in names[i:i + 3])
    assert np.all(Vv["tdnn/vlad/vlad_weight_affine/bias"] != 0) and np.abs(Vv["tdnn/vlad/vlad_centers"]).max() <= np.sqrt(6.0 / 53) + 1e-6
    stat = E.Engine(E.make_config(30, 37, num_nodes_pooling_layer=48, num_nodes_last_layer=64, max_batch=4, max_frames=30, precision="f32"))
    # the two [B T, C] tensors statistics pooling never writes (the activation is allocated either way; the value path of d x is not)
    assert eng.arena_bytes - stat.arena_bytes >= 4 * (30 - 14) * 48 * 4
    stat.close()
    eng.close()


@pytest.mark.parametrize("final", [False, True], ids=["plain", "final_l2"])
@pytest.mark.parametrize("opt", ["sgd", "adam"])
def test_two_steps_match_the_composed_oracle(vlad_oracle, opt, final):
    B, T, P, K, G = 4, 27, 48, 3, 2
    kw = dict(loss_func="softmax", optimizer=opt)
    eng, cfg_o, Vv = make(kw, B, T, P, K, G, final)
    vlad_oracle.update(k=K, final=final)
    rs = np.random.RandomState(42)
    opt_state = {}
    lr = 0.05 if opt == "sgd" else 0.001
    for it in range(2):
        x = rs.randn(B, T, 30).astype(np.float32)
        labels = rs.randint(0, cfg_o.num_speakers, B).astype(np.int32)
        eng.forward(x, True)
        eng.loss(labels, it, True)
        eng.backward(-1)
        vlad_oracle["V"] = Vv
        newV, opt_state, info = TE.oracle_step_with_gpu_relu_pattern(eng, Vv, cfg_o, x.astype(np.float64), labels, lr, it, opt_state)
        for name, shape in (("vlad_weights", (B * (T - 14), K + G)), ("vlad_centers", (K + G, P))):
            assert tuple(eng.endpoint(name).shape) == shape
        a = eng.endpoint("vlad_weights").cpu().numpy()
        assert TE.rel_err(a, V.softmax(info["endpoints"]["tdnn5_relu"].reshape(-1, P) @ Vv["tdnn/vlad/vlad_weight_affine/kernel"]
                                       + Vv["tdnn/vlad/vlad_weight_affine/bias"])) <= 5e-5
        # (applies the update)  The variables after Adam's second update are held to 1e-4 of the tensor, what tests/test_gpu_engine.py asks of
        # variables after a second update (test_second_step_uses_updated_weights_and_staged_backward); its 2e-5 is for a first update, where
        # Adam's step lr g / (|g| + eps) does not depend on the size of g - from t = 2 on it moves with g2 / g1 element by element, so an
        # element whose gradient is 1e-3 of the tensor's largest carries the gradient tolerance (1e-4 of the largest) as 10 % of its step
        TE.compare_step_with_oracle(eng, cfg_o, newV, info, lr, var_tol=1e-4 if (opt == "adam" and it == 1) else 2e-5)
        # the second step is compared from the same state on both sides: the engine's float32 variables and Adam slots after its first
        # update (weight copies rebuilt, t = 2) - the gradients of each step are then held to the one-step tolerance, not to two steps' rounding
        Vv = TE.OrderedDictF64(eng.get_variables())
        if opt == "adam":
            slots = eng.opt_state.cpu().numpy().astype(np.float64)
            for name, (shape, off, trainable) in eng.table.items():
                if trainable:
                    n = int(np.prod(shape)) if len(shape) else 1
                    opt_state[name] = (slots[off:off + n].reshape(shape), slots[eng.n_train + off:eng.n_train + off + n].reshape(shape))
    eng.close()


def test_full_width_step_matches_the_composed_oracle(vlad_oracle):
    B, T, P, K, G = 2, 22, 1500, 8, 2
    eng, cfg_o, Vv = make(dict(loss_func="additive_margin_softmax", margin_m=0.2, last_layer_linear=True), B, T, P, K, G, True, L=512)
    vlad_oracle.update(k=K, final=True, V=Vv)
    rs = np.random.RandomState(1)
    x = rs.randn(B, T, 30).astype(np.float32)
    labels = rs.randint(0, cfg_o.num_speakers, B).astype(np.int32)
    eng.forward(x, True)
    eng.loss(labels, 1234, True)
    eng.backward(-1)
    g1 = eng.grads.clone()
    eng.backward(-1)
    assert (g1 == eng.grads).all(), "two backward passes differ"
    newV, _, info = TE.oracle_step_with_gpu_relu_pattern(eng, Vv, cfg_o, x.astype(np.float64), labels, 0.05, 1234, {})
    TE.compare_step_with_oracle(eng, cfg_o, newV, info, 0.05)
    eng.close()


def test_forward_lengths_matches_one_at_a_time_and_the_oracle(vlad_oracle):
    from tf_kaldi_speaker_amd import engine as E
    lens = [15, 25, 137, 64]
    T, K, G = max(lens), 8, 2
    eng = E.Engine(E.make_config(30, 0, max_batch=len(lens), max_frames=T, pooling_type="ghost_vlad", vlad_num_centers=K, vlad_num_ghosts=G,
                                 vlad_final_l2_norm=True, precision="f32"))
    eng.init_variables(seed=0)
    Vv = eng.get_variables()
    rs = np.random.RandomState(7)
    for k in Vv:
        if k.endswith("moving_mean"):
            Vv[k] = rs.randn(*Vv[k].shape) * 0.1
        if k.endswith("moving_variance"):
            Vv[k] = 0.5 + rs.rand(*Vv[k].shape)
    eng.set_variables({k: v.astype(np.float32) for k, v in Vv.items()})
    Vv = TE.OrderedDictF64(eng.get_variables())
    vlad_oracle.update(k=K, final=True, V=Vv)
    cfg_o = O.Config(feat_dim=30, num_speakers=0)
    utts = [rs.randn(n, 30).astype(np.float32) for n in lens]
    x = np.full((len(lens), T, 30), 1e3, np.float32)              # the padding is not zero: it must not reach any utterance's embedding
    for i, u in enumerate(utts):
        x[i, :len(u)] = u
    eng.forward_lengths(x, np.asarray(lens, np.int32))
    got = {n: eng.endpoint(n).cpu().numpy() for n in ("pooling", "tdnn6_dense", "tdnn7_dense", "output")}
    assert got["pooling"].shape == (len(lens), K * 1500)
    for i, u in enumerate(utts):
        eng.forward(u[None], False)
        _, ep, _ = O.tdnn_forward(Vv, u[None].astype(np.float64), cfg_o, False)
        for name in got:
            one = eng.endpoint(name).cpu().numpy()[0]
            assert TE.rel_err(got[name][i], one.astype(np.float64)) <= 1e-6, (i, name)
            assert TE.rel_err(got[name][i], ep[name][0]) <= 5e-5, (i, name, TE.rel_err(got[name][i], ep[name][0]))
    eng.close()


def test_config_without_the_vlad_fields_is_still_accepted():
    """A host built against xv_config as it was before the three fields were added at its end (struct_bytes = their offset) creates a
    statistics-pooling engine as before; any other size is refused (tests/test_abi.py)."""
    import ctypes as C
    from tf_kaldi_speaker_amd import _lib, engine as E
    c = E.make_config(30, 10, max_batch=2, max_frames=20, precision="f32")
    c.vlad_num_centers, c.vlad_num_ghosts = 77, -5      # beyond the older struct's end: not read
    c.struct_bytes = _lib.XvConfig.vlad_num_centers.offset
    assert c.struct_bytes == C.sizeof(_lib.XvConfig) - 12
    h = C.c_void_p()
    lib = _lib.load()
    _lib.check(lib.xv_engine_create(C.byref(c), C.byref(h)), "xv_engine_create")
    n = lib.xv_engine_num_variables(h)
    lib.xv_engine_destroy(h)
    full = E.Engine(E.make_config(30, 10, max_batch=2, max_frames=20, precision="f32"))
    assert n == len(full.table) and not any("vlad" in k for k in full.table)
    full.close()


def test_refusals_by_name():
    from tf_kaldi_speaker_amd import _lib, engine as E
    with pytest.raises(NotImplementedError, match="precision f16x3 is not supported"):
        E.make_config(30, 10, pooling_type="ghost_vlad", vlad_num_centers=8, vlad_num_ghosts=2, precision="f16x3")
    for k, g in ((0, 2), (8, -1), (60, 5)):
        with pytest.raises(NotImplementedError, match="vlad_num_centers >= 1, vlad_num_ghosts >= 0 and at most 64 clusters"):
            E.make_config(30, 10, pooling_type="ghost_vlad", vlad_num_centers=k, vlad_num_ghosts=g, precision="f32")
    # ... and by the library itself, for a host that fills xv_config on its own
    c = E.make_config(30, 10, pooling_type="ghost_vlad", vlad_num_centers=8, vlad_num_ghosts=2, precision="f32", max_batch=2, max_frames=20)
    c.vlad_num_centers = 63
    with pytest.raises(_lib.XvError, match="at most 64 clusters in all \\(got 63 \\+ 2\\)"):
        E.Engine(c)
    c.vlad_num_centers, c.precision = 8, _lib.PRECISIONS["f16x3"]
    with pytest.raises(_lib.XvError, match="ghost_vlad pooling runs in precision f32 only"):
        E.Engine(c)
