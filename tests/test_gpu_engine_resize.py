"""Growing an engine keeps its state: a Trainer that outgrows its capacity mid-training, and tdnn() re-entered with a longer batch, continue
bit for bit like a fresh engine of the larger capacity that was handed the state.  Growth is DEFINED here as "a fresh engine with the state
copied" - nothing assumes that the arithmetic is independent of the capacity.

Smallest shapes that reach the code: 30-dimensional features, 10 speakers, 2 -> 4 chunks, 24 -> 40 frames (the receptive field is 15, so 24
frames leave 10)."""
import numpy as np
import pytest
import torch

from test_gpu_trainer import CONFIG

pytestmark = pytest.mark.gpu

FROZEN = ["tdnn3_conv/kernel", "tdnn2_bn/moving_mean"]


def _params(**more):
    from tf_kaldi_speaker_amd.misc.utils import ParamsPlain
    p = ParamsPlain()
    p.dict.update(CONFIG, **more)
    return p


def _batches():
    rs = np.random.RandomState(11)
    return [(rs.randn(b, t, 30).astype(np.float32), rs.randint(0, 10, b).astype(np.int32)) for b, t in ((2, 24), (2, 24), (4, 40), (4, 40))]


def _state(eng):
    torch.cuda.synchronize()
    return eng.get_variables(), eng.opt_state.cpu().numpy().copy(), eng.get_gradients()


def _same(a, b, what):
    for (va, oa, ga), (vb, ob, gb) in [(a, b)]:
        assert list(va) == list(vb) and list(ga) == list(gb)
        for k in va:
            assert np.array_equal(va[k], vb[k]), "%s: variable %s" % (what, k)
        for k in ga:
            assert np.array_equal(ga[k], gb[k]), "%s: gradient %s" % (what, k)
        assert oa.shape == ob.shape and np.array_equal(oa, ob), "%s: optimiser state" % what


def test_trainer_growth_is_a_fresh_engine_with_the_state_copied(tmp_path):
    from tf_kaldi_speaker_amd import engine as E
    from tf_kaldi_speaker_amd.model.tdnn import engine_config
    from tf_kaldi_speaker_amd.model.trainer import Trainer
    more = dict(optimizer="adam", num_speakers_per_batch=2, num_segments_per_speaker=1, max_segment_len=24, seed=5)
    tr = Trainer(_params(**more), str(tmp_path / "exp"))
    tr.build("train", dim=30, loss_type="additive_margin_softmax", num_speakers=10, noupdate_var_list=FROZEN)
    cfg = tr.engine.config
    assert (cfg.max_batch, cfg.max_frames) == (2, 24) and tr.engine.n_opt == 2 * tr.engine.n_train
    assert set(tr.engine.frozen_names) == {"tdnn/tdnn3_conv/kernel", "tdnn/tdnn2_bn/moving_mean"}
    batches = _batches()
    start = tr.engine.get_variables()
    for step, (x, y) in enumerate(batches[:2]):
        tr._ensure_capacity(x.shape[0], x.shape[1])
        tr.engine.train_step(x, y, 0.01, step)
    small = tr.engine
    assert tr.engine.config.max_batch == 2 and tr.engine.update_count == 2
    # the hand-over, by hand, at the moment of growth
    variables, opt, count, frozen = small.get_variables(), small.opt_state.clone(), small.update_count, small.frozen_names
    assert np.array_equal(variables["tdnn/tdnn3_conv/kernel"], start["tdnn/tdnn3_conv/kernel"])
    assert not np.array_equal(variables["tdnn/tdnn4_dense/kernel"], start["tdnn/tdnn4_dense/kernel"]) and float(opt.abs().max()) > 0
    tr._ensure_capacity(4, 40)
    grown = tr.engine
    assert grown is not small and (grown.config.max_batch, grown.config.max_frames) == (4, 48)      # frames double, up to 20 000
    other = E.Engine(engine_config(_params(**more), 30, 10, "additive_margin_softmax", grown.config.max_batch, grown.config.max_frames),
                     device=tr.device)
    try:
        assert other.table == grown.table and other.n_opt == grown.n_opt
        other.set_variables(variables)
        other.opt_state.copy_(opt)
        other.update_count = count
        other.set_update_filter(frozen)
        assert grown.update_count == count and grown.frozen_names == frozen
        _same(_state(grown)[:2] + ({},), _state(other)[:2] + ({},), "at the hand-over")
        for step, (x, y) in enumerate(batches[2:], 2):
            tr._ensure_capacity(x.shape[0], x.shape[1])
            assert tr.engine is grown
            grown.train_step(x, y, 0.01, step)
            other.train_step(x, y, 0.01, step)
            _same(_state(grown), _state(other), "step %d" % step)
        assert grown.update_count == other.update_count == 4
        end = grown.get_variables()
        assert np.array_equal(end["tdnn/tdnn3_conv/kernel"], start["tdnn/tdnn3_conv/kernel"])
        assert not np.array_equal(end["tdnn/tdnn4_dense/kernel"], variables["tdnn/tdnn4_dense/kernel"])
    finally:
        other.close()
        tr.close()


def test_tdnn_growth_returns_what_a_graph_created_at_that_size_returns():
    from tf_kaldi_speaker_amd.model import tdnn as T
    rs = np.random.RandomState(12)
    short, long_ = rs.randn(2, 24, 30).astype(np.float32), rs.randn(4, 40, 30).astype(np.float32)
    T.reset_default_graph()
    try:
        T.tdnn(short, _params(seed=7), is_training=False)
        with pytest.raises(ValueError, match="already exists"):
            T.tdnn(short, _params(seed=7), is_training=False)
        out, endpoints = T.tdnn(long_, _params(seed=7), is_training=False, reuse_variables=True)
        grown = {k: v.cpu().numpy() for k, v in endpoints.items()}
        grown_out = out.cpu().numpy()
        T.reset_default_graph()
        out, endpoints = T.tdnn(long_, _params(seed=7), is_training=False)
        assert list(endpoints) == list(grown) and list(grown)[-1].startswith("tdnn7_") and grown["tdnn5_relu"].shape == (4, 26, 1500)
        for k, v in endpoints.items():
            assert np.array_equal(v.cpu().numpy(), grown[k]), k
        assert np.array_equal(out.cpu().numpy(), grown_out) and np.abs(grown_out).max() > 0
    finally:
        T.reset_default_graph()
