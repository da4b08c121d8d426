"""CPU tests of the host layer in front of the pipeline kernels (tf_kaldi_speaker_amd/_host.py and what the drivers in misc/ build on it).

The batch boundaries below are literals recorded from the drivers as they stood before they shared one batcher: a changed boundary
changes what the shape-dependent kernels (augmentation, the MFCC row batches, the cohort statistics in tiles) compute, bit for bit."""
import numpy as np
import pytest

from tf_kaldi_speaker_amd import _host, ops
from tf_kaldi_speaker_amd.misc import augment, backend, features, scoring


# ---- greedy batches -------------------------------------------------------------------------------------------------------------
def _extractor(workspace_bytes):
    """A FeatureExtractor without its constructor's upload: _batches is host arithmetic."""
    fx = object.__new__(features.FeatureExtractor)
    fx.ops, fx.mfcc, fx.workspace_bytes = ops, features.MfccOptions(), workspace_bytes
    fx.cfg = fx.mfcc.config()
    return fx


def _extractor_case():
    rs = np.random.RandomState(7)
    lengths = [int(n) for n in rs.randint(0, 48001, 40)]          # 0 .. 3 s at 16 kHz
    for i in (0, 3, 4, 17, 39):
        lengths[i] = 0
    lengths[9] = 60                                                  # samples, but no frame
    fx = _extractor(0)
    return lengths, [fx.num_frames(n) for n in lengths]


EXTRACT_BATCHES = [[0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14], [15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25], [26, 27, 28, 29, 30, 31, 32, 33, 34, 35],
                   [36, 37, 38, 39]]
EXTRACT_TIGHT = [[0], [1], [2, 3, 4, 5], [6], [7], [8], [9], [10], [11, 12, 13], [14, 15], [16, 17], [18], [19], [20], [21], [22], [23]]
EXTRACT_REFUSAL = "FeatureExtractor: a workspace of 130000 bytes does not hold utterance 26 (47305 samples, 296 frames: 130426 bytes)"


def test_feature_extractor_batches_are_the_recorded_ones():
    lengths, frames = _extractor_case()
    assert frames[0] == 0 and frames[9] == 0 and max(frames) > 250
    assert list(_extractor(1000000)._batches(frames, lengths)) == EXTRACT_BATCHES
    got = []
    with pytest.raises(ValueError) as e:
        for batch in _extractor(130000)._batches(frames, lengths):
            got.append(batch)
    assert got == EXTRACT_TIGHT and str(e.value) == EXTRACT_REFUSAL


def test_feature_extractor_batches_hold_at_most_65535_utterances():
    n = 2 * 65535 + 3
    sizes = [len(b) for b in _extractor(1 << 40)._batches([0] * n, [0] * n)]
    assert sizes == [65535, 65535, 3]
    sizes = [len(b) for b in _host.greedy_batches(n, lambda i, *totals: (), lambda: 0, 1, max_items=65535)]
    assert sizes == [65535, 65535, 3]


def _augmenter(workspace_bytes):
    """An Augmenter without its constructor's uploads: _batches is host arithmetic (xv_augment_workspace_bytes makes no GPU call)."""
    aug = object.__new__(augment.Augmenter)
    aug.ops, aug.workspace_bytes, aug.tile = ops, workspace_bytes, ops.augment_plan(1)["tile"]
    return aug


def _augmenter_case():
    rs = np.random.RandomState(11)
    n = rs.randint(1, 48001, 30).astype(np.int64)
    taps = np.asarray([0, 4000, 16000], np.int64)[rs.randint(0, 3, 30)]
    entries = [augment.PlanEntry("utt%02d-aug" % i, "utt%02d" % i, rir="r%d" % t if t else None, noises=[("n", 10.0, 0, False)] * int(k))
               for i, (t, k) in enumerate(zip(taps, rs.randint(0, 4, 30)))]
    return n, np.where(taps > 0, n + taps - 1, n), entries


AUGMENT_BATCHES = [[0, 1, 2, 3, 4, 5, 6, 7], [8, 9, 10, 11, 12, 13, 14], [15, 16, 17, 18, 19, 20, 21, 22, 23], [24, 25, 26, 27, 28, 29]]
AUGMENT_TIGHT = [[0], [1], [2, 3]]
AUGMENT_REFUSAL = "Augmenter: a workspace of 287000 bytes does not hold utterance 5 (utt05-aug: 36792 samples under 16000 taps: 287440 bytes)"


def test_augmenter_batches_are_the_recorded_ones():
    n, m, entries = _augmenter_case()
    assert list(_augmenter(1500000)._batches(n, m, entries)) == AUGMENT_BATCHES
    got = []
    with pytest.raises(ValueError) as e:
        for batch in _augmenter(287000)._batches(n, m, entries):
            got.append(batch)
    assert got == AUGMENT_TIGHT and str(e.value) == AUGMENT_REFUSAL


def test_greedy_batches_refuses_before_it_grows_and_passes_the_totals_on():
    seen = []

    def grow(i, count=0, total=0):
        seen.append((i, count, total))
        return count + 1, total + i

    cost_of, too_big = lambda count, total: total, lambda i, cost: "item %d: %d" % (i, cost)
    assert list(_host.greedy_batches(6, grow, cost_of, 5, too_big=too_big)) == [[0, 1, 2], [3], [4], [5]]
    assert (3, 3, 3) in seen and (3, 0, 0) in seen                 # item 3 was tried on top of 0 + 1 + 2, and alone
    with pytest.raises(ValueError, match="^item 6: 6$"):
        list(_host.greedy_batches(7, grow, cost_of, 5, too_big=too_big))
    assert list(_host.greedy_batches(0, grow, cost_of, 5)) == []


# ---- fixed steps ----------------------------------------------------------------------------------------------------------------
class _Host(object):
    """What a fake kernel call returns: .cpu().numpy() of the scorers' loops."""

    def __init__(self, a):
        self.a = a

    def cpu(self):
        return self

    def numpy(self):
        return self.a


class _FakeOps(object):
    def __init__(self):
        self.calls = []

    def score_trials(self, e, t, d, ei, ti, e_stats=None, t_stats=None):
        self.calls.append((int(ei[0]), int(ti[-1]), len(ei)))
        return _Host(np.asarray(ei, np.float32))

    def backend_plda_trials(self, e, t, d, ei, ti, nidx, coef, g, k0):
        self.calls.append((int(ei[0]), int(ti[-1]), len(ei)))
        return _Host(np.asarray(ti, np.float32))

    def score_cohort_workspace_bytes(self, rows, n_cohort, d):
        return rows * n_cohort * 4

    def score_cohort_stats(self, x, cohort, d, top_k, ws_bytes=None):
        import torch
        self.calls.append((x.shape[0], ws_bytes))
        return torch.stack([x[:, 0], x[:, 0]], dim=1)


def test_trial_batches_are_workspace_bytes_over_12():
    import torch
    ei, ti = np.arange(25), np.arange(100, 125)
    s = object.__new__(scoring.CosineScorer)
    s.torch, s.ops, s.workspace_bytes, s.d, s._cohort = torch, _FakeOps(), 131, 8, None
    assert np.array_equal(s.score(None, None, ei, ti), ei.astype(np.float32))
    assert s.ops.calls == [(0, 109, 10), (10, 119, 10), (20, 124, 5)]
    s.ops.calls, s.workspace_bytes = [], 12 * 25
    assert s.score(None, None, ei, ti).shape == (25,) and s.ops.calls == [(0, 124, 25)]
    s.ops.calls, s.workspace_bytes = [], 5                          # fewer than one trial's bytes: one trial per call
    assert s.score(None, None, ei[:3], ti[:3]).shape == (3,) and s.ops.calls == [(0, 100, 1), (1, 101, 1), (2, 102, 1)]

    b = object.__new__(backend.BackendScorer)
    b.torch, b.ops, b.device, b.workspace_bytes, b.dim, b.mode = torch, _FakeOps(), torch.device("cpu"), 131, 8, "lda_cos"
    assert np.array_equal(b.score(None, None, ei, ti), ei.astype(np.float32))
    assert b.ops.calls == [(0, 109, 10), (10, 119, 10), (20, 124, 5)]
    b.ops.calls, b.mode = [], "plda"
    b.backend = backend.Backend(np.zeros(8, np.float32), None, dict(mean=np.zeros(8), transform=np.eye(8), psi=np.linspace(2.0, 0.1, 8)))
    assert np.array_equal(b.score(torch.zeros(4, 8), None, ei % 4, ti, enrol_n=[1, 3, 3, 2]), ti.astype(np.float32))
    assert b.ops.calls == [(0, 109, 10), (2, 119, 10), (0, 124, 5)]


def test_cohort_row_batches_are_whole_128_row_tiles_of_the_workspace():
    import torch
    s = object.__new__(scoring.CosineScorer)
    s.torch, s.ops, s.d, s.top_k, s._cohort = torch, _FakeOps(), 8, 3, torch.zeros(50, 8)
    x = torch.arange(300, dtype=torch.float32)[:, None].repeat(1, 8)
    tile = 128 * 50 * 4
    s.workspace_bytes = 2 * tile + 5
    assert torch.equal(s._stats(x)[:, 0], x[:, 0])
    assert s.ops.calls == [(256, 256 * 50 * 4), (44, 44 * 50 * 4)]
    s.ops.calls, s.workspace_bytes = [], 3 * tile
    assert s._stats(x).shape == (300, 2) and s.ops.calls == [(300, 300 * 50 * 4)]
    s.workspace_bytes = tile - 1
    with pytest.raises(ValueError, match="CosineScorer: a workspace of %d bytes does not hold one 128-row tile of 50 cohort scores \\(%d bytes\\)" % (tile - 1, tile)):
        s._stats(x)


def test_transform_chain_runs_in_batches_of_prepare_rows(monkeypatch):
    import torch
    monkeypatch.setattr(backend, "PREPARE_ROWS", 4)
    chain = object.__new__(backend._Chain)
    chain.torch, seen = torch, []
    chain.unit = lambda x: seen.append(("unit", x.shape[0])) or x
    chain.plda = lambda y, n_utts=None: seen.append(("plda", None if n_utts is None else list(n_utts))) or y + 1
    x = torch.arange(10, dtype=torch.float32)[:, None]
    assert torch.equal(chain.run(x, False), x) and seen == [("unit", 4), ("unit", 4), ("unit", 2)]
    del seen[:]
    assert torch.equal(chain.run(x, True, np.arange(10)), x + 1)
    assert seen == [("unit", 4), ("plda", [0, 1, 2, 3]), ("unit", 4), ("plda", [4, 5, 6, 7]), ("unit", 2), ("plda", [8, 9])]
    assert chain.run(x[:3], False) is not None and _host.cat([x]) is x


def test_steps_and_cat():
    import torch
    assert list(_host.steps(10, 4)) == [(0, 4), (4, 8), (8, 10)] and list(_host.steps(8, 4)) == [(0, 4), (4, 8)]
    assert list(_host.steps(0, 4)) == [] and list(_host.steps(3, 100)) == [(0, 3)]
    a = np.arange(3)
    assert _host.cat([a]) is a and np.array_equal(_host.cat([a, a]), np.r_[a, a])
    t = torch.arange(3)
    assert _host.cat([t]) is t and torch.equal(_host.cat([t, t]), torch.cat([t, t]))
    with pytest.raises(ValueError):
        _host.cat([])                                               # no trials: what numpy.concatenate says


# ---- host integer arrays ----------------------------------------------------------------------------------------------------------
def test_host_ints_takes_what_each_call_site_takes():
    ints = _host.host_ints
    a = ints([3, 1, 2], "x")
    assert isinstance(a, np.ndarray) and a.tolist() == [3, 1, 2]
    assert ints(np.arange(3, dtype=np.uint8), "x").dtype == np.uint8            # the dtype is the caller's
    assert ints(np.zeros(0, np.int32), "x", dtype=np.int64).dtype == np.int64 and ints(np.zeros(0, np.int32), "x").size == 0     # empty is a length
    # augment: any length or exactly n, empty allowed; one message
    for bad in (np.zeros((2, 2), np.int64), np.zeros(3), 5, np.zeros(3, bool)):
        with pytest.raises(ValueError, match="^augment: src_off must be a 1-D integer array$"):
            ints(bad, "augment: src_off")
    for bad in ([1, 2], [1, 2, 3, 4], np.zeros(3), np.zeros((3, 1), np.int32)):
        with pytest.raises(ValueError, match="^augment: utt_rir must be a 1-D integer array of 3$"):
            ints(bad, "augment: utt_rir", n=3)
    assert ints([1, 2, 3], "augment: utt_rir", n=3, dtype=np.int64).dtype == np.int64
    # the back end: non-empty, inside [lo, hi); the dtype is kept
    for bad in ([], np.zeros((1, 1), np.int32), [0.5]):
        with pytest.raises(ValueError, match="^backend_plda_trials: ei must be a non-empty 1-D integer array$"):
            ints(bad, "backend_plda_trials: ei", min_size=1, lo=0, hi=4)
    for bad in ([-1, 0], [0, 4]):
        with pytest.raises(IndexError, match="^backend_plda_trials: ei holds a value outside 0 \\.\\. 3$"):
            ints(bad, "backend_plda_trials: ei", min_size=1, lo=0, hi=4)
    assert ints(np.asarray([0, 3], np.int16), "e", min_size=1, lo=0, hi=4).dtype == np.int16
    with pytest.raises(IndexError, match="^backend_plda_normalize: n_utts holds a value outside 1 \\.\\. 2147483647$"):
        ints([0], "backend_plda_normalize: n_utts", min_size=1, lo=1, hi=1 << 31)
    with pytest.raises(IndexError, match="outside 1 .. 2147483647"):
        ints([1 << 31], "n", min_size=1, lo=1, hi=1 << 31)
    # pairs with a message of their own (mfcc, score_trials), CSR offsets (backend_group_means: at least two entries)
    pair = "score_trials: ei and ti must be two non-empty 1-D integer arrays of one length"
    for bad in ([], [[0]], [0.0]):
        with pytest.raises(ValueError, match="^%s$" % pair):
            ints(bad, min_size=1, msg=pair)
    with pytest.raises(ValueError, match="^%s$" % pair):
        ints([0, 1], n=3, msg=pair)
    for bad in ([0], [], [[0, 1]], [0.0, 1.0]):
        with pytest.raises(ValueError, match="^offsets: as stated$"):
            ints(bad, min_size=2, msg="offsets: as stated")
    assert ints(np.zeros(0, np.int64), "x", lo=0, hi=1).size == 0                 # no value, none outside


def test_pipeline_ops_refuse_host_arrays_as_before():
    """The refusals that come before any device is touched, through the public names (tensors on the CPU: nothing is launched)."""
    import torch
    e = torch.zeros(3, 8)
    for ei, ti in (([], []), ([0, 1], [0]), ([[0]], [[0]]), ([0.0], [0])):
        with pytest.raises(ValueError, match="^score_trials: ei and ti must be two non-empty 1-D integer arrays of one length$"):
            ops.score_trials(e, e, 8, ei, ti)
    with pytest.raises(IndexError, match="^score_trials: ei holds an index outside 0 \\.\\. 2$"):
        ops.score_trials(e, e, 8, [3], [0])
    with pytest.raises(IndexError, match="^score_trials: ti holds an index outside 0 \\.\\. 2$"):
        ops.score_trials(e, e, 8, [0], [-1])
    with pytest.raises(ValueError, match="two non-empty"):          # both shapes are looked at before any index
        ops.score_trials(e, e, 8, [7], [[0]])
    pcm = torch.zeros(100, dtype=torch.int16)
    for off, n in (([], []), ([0], [1, 2]), ([0.0], [1])):
        with pytest.raises(ValueError, match="^mfcc: offsets and samples must be two non-empty 1-D integer arrays of one length$"):
            ops.mfcc(None, None, pcm, off, n)
    for off, n in (([-1], [5]), ([0], [-1]), ([90], [11])):
        with pytest.raises(IndexError, match="^mfcc: an utterance lies outside the 100 samples of pcm$"):
            ops.mfcc(None, None, pcm, off, n)
    for off in ([0], [1, 2], [[0, 2]], [0.0, 2.0]):
        with pytest.raises(ValueError, match="^backend_group_means: offsets must be a 1-D integer array \\[groups \\+ 1\\] that starts at 0$"):
            ops.backend_group_means(e, 8, off, [0, 1])
    with pytest.raises(ValueError, match="^backend_group_means: group 1 is empty$"):
        ops.backend_group_means(e, 8, [0, 1, 1], [0])
    with pytest.raises(ValueError, match="^backend_group_means: rows must be a non-empty 1-D integer array$"):
        ops.backend_group_means(e, 8, [0, 2], [])
    with pytest.raises(IndexError, match="^backend_group_means: rows holds a value outside 0 \\.\\. 2$"):
        ops.backend_group_means(e, 8, [0, 2], [0, 3])
    with pytest.raises(ValueError, match="^backend_group_means: offsets end at 2, rows holds 3 indices$"):
        ops.backend_group_means(e, 8, [0, 2], [0, 1, 2])
    psi = torch.ones(8)
    with pytest.raises(IndexError, match="^backend_plda_normalize: n_utts holds a value outside 1 \\.\\. 2147483647$"):
        ops.backend_plda_normalize(e, 8, psi, n_utts=[1, 0, 1])
    with pytest.raises(ValueError, match="^backend_plda_normalize: n_utts must hold one count per row \\(3, got 2\\)$"):
        ops.backend_plda_normalize(e, 8, psi, n_utts=[1, 1])
    with pytest.raises(ValueError, match="^backend_plda_normalize: psi must be 8 contiguous float32 values$"):
        ops.backend_plda_normalize(e, 8, torch.ones(7))
    with pytest.raises(ValueError, match="^score_prepare: mean must be 8 contiguous float32 values$"):
        ops.score_prepare(e, mean=torch.ones(8, dtype=torch.float64))
    with pytest.raises(ValueError, match="^backend_center: mean must be 8 contiguous float32 values$"):
        ops.backend_center(e, mean=torch.ones(16)[::2])
    with pytest.raises(ValueError, match="^backend_scatter: mean must be 6 contiguous float32 values$"):
        ops.backend_scatter(e, d=6, mean=torch.ones(8))
    whole = torch.zeros(3, 12)
    for name, call in (("score_prepare", lambda: ops.score_prepare(e, out=whole[:, :8])), ("backend_center", lambda: ops.backend_center(e, out=whole[:, :8])),
                       ("backend_plda_normalize", lambda: ops.backend_plda_normalize(e, 8, psi, out=whole[:, :8]))):
        with pytest.raises(ValueError, match="^%s: out must be the whole \\[rows, pitch\\] buffer \\(its padding columns are written\\)$" % name):
            call()
    coef, g, k0 = torch.zeros(2, 2, 8), torch.zeros(8), torch.zeros(2)
    with pytest.raises(IndexError, match="^backend_plda_trials: nidx holds a value outside 0 \\.\\. 1$"):
        ops.backend_plda_trials(e, e, 8, [0], [0], [0, 1, 2], coef, g, k0)
    with pytest.raises(ValueError, match="^backend_plda_trials: ei and ti must be of one length, nidx one entry per enrol row$"):
        ops.backend_plda_trials(e, e, 8, [0], [0, 1], [0, 1, 1], coef, g, k0)
    src = torch.ones(50, dtype=torch.int16)
    cfg = ops.augment_config()
    with pytest.raises(ValueError, match="^augment: src_len must be a 1-D integer array$"):
        ops.augment(cfg, src, [0], [5.0])
    with pytest.raises(ValueError, match="^augment: src_off and src_len must be two non-empty arrays of one length$"):
        ops.augment(cfg, src, np.zeros(0, np.int64), np.zeros(0, np.int64))
    with pytest.raises(ValueError, match="^augment: utt_rir must be a 1-D integer array of 1$"):
        ops.augment(cfg, src, [0], [5], utt_rir=[0, 0])
    with pytest.raises(IndexError, match="^augment: a source is empty or lies outside the 50 samples of src$"):
        ops.augment(cfg, src, [48], [5])
    with pytest.raises(ValueError, match="^augment: nz_first must be a 1-D integer array of 2$"):
        ops.augment(cfg, src, [0], [5], nz_first=[0])
    with pytest.raises(ValueError, match="^augment: out_offsets must be a 1-D integer array of 1$"):
        ops.augment(cfg, src, [0], [5], out_offsets=[[0]])


def test_wave_ops_refuse_as_before():
    """The refusals of the ops that take PCM, and of cm_decode_ragged, that only GPU tests reached: texts and exception types, byte for
    byte (tensors on the CPU: nothing is launched)."""
    import torch
    pcm, one = torch.zeros(100, dtype=torch.int16), ([0], [10])
    cfg = ops.resample_config(16000, 8000)
    tables = torch.from_numpy(ops.resample_tables(cfg))
    with pytest.raises(ValueError, match="^resample: offsets and samples must be two non-empty 1-D integer arrays of one length$"):
        ops.resample(cfg, tables, pcm, [], [])
    with pytest.raises(IndexError, match="^resample: an utterance lies outside the 100 samples of pcm$"):
        ops.resample(cfg, tables, pcm, [90], [11])
    with pytest.raises(ValueError, match="^resample: tables must be resample_tables\\(cfg\\) as a contiguous float32 device tensor of 27 values$"):
        ops.resample(cfg, tables[:-1].clone(), pcm, *one)
    with pytest.raises(IndexError, match="^resample: the outputs overlap or lie outside the 8 samples of out_pcm$"):
        ops.resample(cfg, tables, pcm, [0, 10], [10, 10], out_offsets=[0, 3])
    with pytest.raises(IndexError, match="^resample: the outputs overlap or lie outside the 2 samples of out_pcm$"):
        ops.resample(cfg, tables, pcm, *one, out_pcm=torch.zeros(2, dtype=torch.int16))
    with pytest.raises(ValueError, match="^resample: out_f32 must be a contiguous 1-D float32 tensor of out_pcm's size$"):
        ops.resample(cfg, tables, pcm, *one, out_f32=torch.zeros(2))
    with pytest.raises(ValueError, match="^resample: pcm must be a contiguous 1-D int16 tensor$"):
        ops.resample(cfg, tables, pcm.float(), *one)
    src, acfg = torch.ones(50, dtype=torch.int16), ops.augment_config()
    with pytest.raises(IndexError, match="^augment: the outputs overlap or lie outside the 13 samples of out_pcm$"):
        ops.augment(acfg, src, [0, 10], [10, 10], out_offsets=[0, 3])
    with pytest.raises(ValueError, match="^augment: out_f32 must be a contiguous 1-D float32 tensor of out_pcm's size$"):
        ops.augment(acfg, src, *one, out_f32=torch.zeros(2))
    with pytest.raises(IndexError, match="^augment: an impulse response is empty or lies outside the 50 samples of rir$"):
        ops.augment(acfg, src, *one, rir=src, rir_off=[45], rir_len=[10], rir_early=[(0, 1, 0)], utt_rir=[0])
    with pytest.raises(IndexError, match="^augment: a noise is empty or lies outside the 50 samples of noise$"):
        ops.augment(acfg, src, *one, noise=src, noise_off=[45], noise_len=[10], nz_first=[0, 1], nz_id=[0], nz_snr=[10.0], nz_start=[0], nz_span=[-1])
    fcfg = ops.fbank_config()
    with pytest.raises(IndexError, match="^fbank: an utterance lies outside the 100 samples of pcm$"):
        ops.fbank(fcfg, None, pcm, [90], [11])
    with pytest.raises(ValueError, match="^fbank: tables must be fbank_tables\\(cfg\\) as a contiguous float32 device tensor$"):
        ops.fbank(fcfg, torch.from_numpy(ops.fbank_tables(fcfg))[:-1].clone(), pcm, *one)
    with pytest.raises(ValueError, match="^fbank: offsets and samples must be two non-empty 1-D integer arrays of one length$"):
        ops.fbank(fcfg, None, pcm, [0], [1, 2])
    with pytest.raises(IndexError, match="^cm_decode_ragged: an image lies outside the 10 bytes of packed$"):
        ops.cm_decode_ragged(torch.zeros(10, dtype=torch.uint8), [0], [3], 3, 2)


class _FakeResampler(object):
    """What a resampler cache hands out: run() records its rate and the lengths it was given and passes the lengths on."""

    def __init__(self, rate, seen):
        self.rate, self.seen = rate, seen

    def run(self, waves):
        n = np.asarray([len(w) for w in waves], np.int64)
        self.seen.append((self.rate, n.tolist()))
        return None, _host.exclusive_offsets(n), n, np.zeros(len(n), np.int64)


def test_rate_groups_are_first_appearance_and_refused_once():
    """extract_at_rates and device_batches visit the sample rates in the order they first appear, the members of a rate in list order;
    a rate the options do not allow is refused with one text."""
    import torch
    rates, seen = [16000, 8000, 16000, 44100, 8000], []
    waves = [np.zeros(100 + i, np.int16) for i in range(5)]             # utterance i is known by its length
    want = [(16000, [100, 102]), (8000, [101, 104]), (44100, [103])]

    def packed(pcm, offsets, lengths, cm_header=None):      # stands in for extract_packed: a result per utterance, its length
        if pcm is not None:                                  # the group at sample_frequency (the fake resamplers hand on no samples)
            seen.append((16000, [int(n) for n in lengths]))
        return [int(n) for n in lengths]

    def extractor(**allow):
        fx = object.__new__(features.FeatureExtractor)
        fx.torch, fx.ops, fx.device, fx.mfcc, fx.workspace_bytes, fx.with_vad = torch, ops, torch.device("cpu"), features.MfccOptions(**allow), 1 << 30, False
        fx.cfg = fx.mfcc.config()
        fx._resamplers = {(rate, fx.mfcc.sample_frequency): _FakeResampler(rate, seen) for rate in (8000, 44100)}
        fx.extract_packed = packed
        fx.on_device = lambda pcm, offsets, lengths, t_out: (torch.zeros(len(lengths), t_out, 1), None, None)
        return fx

    fx = extractor(allow_downsample=1, allow_upsample=1)
    assert fx.extract_at_rates(waves, rates) == [100, 101, 102, 103, 104] and seen == want
    del seen[:]
    got = [(members, list(samples)) for members, samples, batch in fx.device_batches(waves, rates)]
    assert got == [([0, 2], [100, 102]), ([1, 4], [101, 104]), ([3], [103])] and seen == want[1:]
    refusal = "^sample rate 8000 Hz, but --sample-frequency=16000 \\(there is no resampling without --allow-upsample=true\\)$"
    for visit in (lambda fx: fx.extract_at_rates(waves, rates), lambda fx: list(fx.device_batches(waves, rates))):
        with pytest.raises(ValueError, match=refusal):
            visit(extractor(allow_downsample=1, allow_upsample=0))


def test_small_helpers():
    import torch
    assert [_host.pitch4(d) for d in (0, 1, 4, 5, 150, 512)] == [0, 4, 4, 8, 152, 512]
    assert _host.exclusive_offsets([3, 0, 5]).tolist() == [0, 3, 3] and _host.exclusive_offsets([7]).tolist() == [0]
    assert _host.exclusive_offsets(np.asarray([2, 2], np.int32)).dtype == np.int64
    assert _host.DEFAULT_WORKSPACE_BYTES == 1 << 30
    assert features.DEFAULT_WORKSPACE_BYTES == augment.DEFAULT_WORKSPACE_BYTES == scoring.DEFAULT_WORKSPACE_BYTES == backend.DEFAULT_WORKSPACE_BYTES == 1 << 30
    up = _host.upload([1, 2, 3], np.int32, "cpu")
    assert up.dtype == torch.int32 and up.tolist() == [1, 2, 3] and _host.upload(np.arange(4)[::2], np.int64, "cpu").is_contiguous()
    t, o, dev = _host.device_ops("cpu")
    assert t is torch and o is ops and dev == torch.device("cpu")
    assert _host.pitched(torch.zeros(3, 12)[:, :8], "x") == (3, 12)
    with pytest.raises(ValueError, match="^x: a 2-D float32 tensor with contiguous rows is expected$"):
        _host.pitched(torch.zeros(3, 12)[:, ::2], "x")


def test_both_import_styles_need_no_gpu():
    """`import tf_kaldi_speaker_amd.ops` and the flat form with the package directory on sys.path (how the drivers under nnet/lib run)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = os.path.join(root, "tf_kaldi_speaker_amd")
    check = ("assert ops.mfcc is w.mfcc and ops.score_trials is p.score_trials and ops._p is h._p and h.device_ops('cpu')[1] is ops; "
             "assert ops.ahc_cluster is d.ahc_cluster and ops.vbx is d.vbx and ops.AHC_MAX_N == d.AHC_MAX_N == diarization.FIRST_PASS_CAP == 2048")
    for path, code in ((root, "import tf_kaldi_speaker_amd.ops as ops, tf_kaldi_speaker_amd.pipeline_ops as p, tf_kaldi_speaker_amd.wave_ops as w, "
                              "tf_kaldi_speaker_amd.diar_ops as d, tf_kaldi_speaker_amd._host as h; "
                              "from tf_kaldi_speaker_amd.misc import features, augment, scoring, backend, diarization; " + check),
                       (pkg, "import ops, pipeline_ops as p, wave_ops as w, diar_ops as d, _host as h; "
                             "from misc import features, augment, scoring, backend, diarization; " + check)):
        r = subprocess.run([sys.executable, "-c", code], cwd="/", env=dict(os.environ, PYTHONPATH=path, HIP_VISIBLE_DEVICES=""), capture_output=True,
                           text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
