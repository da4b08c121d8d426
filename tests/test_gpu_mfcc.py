"""xv_mfcc and xv_energy_vad on a real MI355X against the fp64 restatement (tests/mfcc_ref.py; Kaldi is not available: parity by restatement).

Tolerance of the features, per utterance and per column class (column 0 - the log-energy, or C0 where use_energy is off - apart from the
cepstral columns): |got - ref| <= 4 * D32 + 2^-21 * |ref|, D32 the largest |fp32 restatement - fp64 restatement| over that utterance and
class: what the number format alone costs there (the signal has a 40 dB dynamic range, so weak mel bins sit beside strong ones), times 4
because the GPU's FFT order and reduction trees differ from pocketfft's, plus two ulps for the last log and the rounding.  It is measured on
the restatement, never on the code under test.  The VAD masks must be EQUAL to the restatement's, after the test has shown on the reference
that no frame's log-energy lies within 1e-2 of the threshold (the features are good to ~1e-6 there)."""
import numpy as np
import pytest

from tests import frontend_ref as F
from tests import mfcc_ref as R

pytestmark = pytest.mark.gpu

LENS = [80, 81, 239, 240, 399, 400, 401, 560, 16000, 48037]
VAD_SECOND = dict(threshold=18.0, mean_scale=0.0, context=0, proportion=1.0)      # between the loud (~21.6) and the quiet (~14.3) stretches


@pytest.fixture(scope="module")
def cases():
    """Per configuration: the waveforms, their fp64 and fp32 restatements; computed once, read only."""
    out = {}
    for name, cfg in R.CONFIGS.items():
        rs = np.random.RandomState(41)
        waves = [R.signal(rs, n, cfg["sample_frequency"]) for n in LENS]
        ref64 = [R.mfcc(w, cfg) for w in waves]
        ref32 = [R.mfcc(w, cfg, np.float32) for w in waves]
        for a in waves + ref64 + ref32:
            a.setflags(write=False)
        out[name] = (cfg, waves, ref64, ref32)
    return out


def _pack(waves):
    """Back to back behind one stray sample: the first offset is odd, so the utterances have no alignment beyond two bytes."""
    offsets = 1 + np.concatenate([[0], np.cumsum([len(w) for w in waves])[:-1]]).astype(np.int64)
    assert offsets[0] % 2 == 1 and len({int(o) % 2 for o in offsets}) == 2
    return np.concatenate([np.array([12345], np.int16)] + list(waves)), offsets


def _run(cfg, waves, t_out):
    import torch
    from tf_kaldi_speaker_amd import ops
    dev = torch.device("cuda:0")
    c = ops.mfcc_config(**cfg)
    tables = torch.from_numpy(ops.mfcc_tables(c)).to(dev)
    buf, offsets = _pack(waves)
    pcm = torch.from_numpy(buf).to(dev)
    lens = np.asarray([len(w) for w in waves], np.int64)
    out, rows = ops.mfcc(c, tables, pcm, offsets, lens, t_out)
    out2, rows2 = ops.mfcc(c, tables, pcm, offsets, lens, t_out)
    torch.cuda.synchronize()
    got, got2 = out.cpu().numpy(), out2.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), got2.view(np.uint32)), "two calls on the same input differ"
    assert np.array_equal(rows.cpu().numpy(), rows2.cpu().numpy())
    return got, rows.cpu().numpy()


def _tolerance(r64, r32, cols):
    d32 = float(np.abs(r32[:, cols].astype(np.float64) - r64[:, cols]).max())
    return d32, 4.0 * d32 + 2.0 ** -21 * np.abs(r64[:, cols])


def _check(name, got, rows, ref64, ref32, t_out):
    worst = 0.0
    ceps = ref64[0].shape[1]
    for i, (r64, r32) in enumerate(zip(ref64, ref32)):
        keep = min(len(r64), t_out)
        assert rows[i] == keep, (i, rows[i], keep)
        assert not got[i, keep:].any(), "utterance %d: rows behind rows_out are not exactly zero" % i
        if keep == 0:
            continue
        assert np.isfinite(got[i, :keep]).all()
        for label, cols in (("col0", slice(0, 1)), ("ceps", slice(1, ceps))):
            d32, tol = _tolerance(r64, r32, cols)
            err = np.abs(got[i, :keep, cols].astype(np.float64) - r64[:keep, cols])
            ratio = float((err / tol[:keep]).max())
            print("%s n=%d T=%d %s: D32 %.3g  max |got - ref| %.3g  max |ref| %.4g  worst error / tolerance %.3f"
                  % (name, LENS[i], len(r64), label, d32, float(err.max()), float(np.abs(r64[:, cols]).max()), ratio))
            worst = max(worst, ratio)
    assert worst <= 1.0, worst


@pytest.mark.parametrize("name", sorted(R.CONFIGS))
def test_mfcc_against_the_restatement(cases, name):
    cfg, waves, ref64, ref32 = cases[name]
    t_out = max(len(r) for r in ref64)
    assert t_out == R.num_frames(48037, cfg) and min(len(r) for r in ref64) == (0 if cfg["snip_edges"] else 1)
    got, rows = _run(cfg, waves, t_out)
    assert got.shape == (len(LENS), t_out, cfg["num_ceps"])
    _check(name, got, rows, ref64, ref32, t_out)
    # t_out below most frame counts: the output is cut, rows_out says so, and a frame's bits do not depend on t_out
    cut, rows_cut = _run(cfg, waves, 7)
    _check(name + " (t_out 7)", cut, rows_cut, ref64, ref32, 7)
    assert np.array_equal(cut.view(np.uint32), got[:, :7].view(np.uint32))


# the two FFT sizes the three configurations leave out: N = 128 (half the lanes idle in the butterflies) with mel bins so narrow at the low
# end that some hold no FFT bin (their energy is the FLT_EPSILON floor), and N = 1024 with L = N (no zero padding) at the limits of the
# table sizes, 128 bins x 128 coefficients (tables + slices = 103 KB of LDS: the launcher raises the kernel's dynamic-LDS limit)
OTHER_SIZES = {"n128": R.config(frame_length_ms=5.0, frame_shift_ms=2.0, num_mel_bins=40, num_ceps=12),
               "n1024": R.config(frame_length_ms=64.0, frame_shift_ms=16.0, num_mel_bins=128, num_ceps=128, snip_edges=1)}
OTHER_LENS = [81, 1023, 1024, 1601, 16000]


@pytest.mark.parametrize("name", sorted(OTHER_SIZES))
def test_mfcc_other_fft_sizes(name):
    cfg = OTHER_SIZES[name]
    assert R.dims(cfg)[2] == int(name[1:])
    rs = np.random.RandomState(53)
    waves = [R.signal(rs, n, 16000.0) for n in OTHER_LENS]
    ref64, ref32 = [R.mfcc(w, cfg) for w in waves], [R.mfcc(w, cfg, np.float32) for w in waves]
    assert (R.tables(cfg)["mel_count"].min() == 0) == (name == "n128")
    if name == "n1024":
        assert [len(r) for r in ref64[:3]] == [0, 0, 1]
    t_out = max(len(r) for r in ref64)
    got, rows = _run(cfg, waves, t_out)
    worst = 0.0
    for i, (r64, r32) in enumerate(zip(ref64, ref32)):
        assert rows[i] == len(r64) and not got[i, len(r64):].any(), i
        for label, cols in (("col0", slice(0, 1)), ("ceps", slice(1, cfg["num_ceps"]))):
            if len(r64) == 0:
                continue
            d32, tol = _tolerance(r64, r32, cols)
            err = np.abs(got[i, :len(r64), cols].astype(np.float64) - r64[:, cols])
            print("%s n=%d T=%d %s: D32 %.3g  max |got - ref| %.3g  worst error / tolerance %.3f"
                  % (name, OTHER_LENS[i], len(r64), label, d32, float(err.max()), float((err / tol).max())))
            worst = max(worst, float((err / tol).max()))
    assert worst <= 1.0, worst


def test_mfcc_refuses_bad_arguments(cases):
    import torch
    from tf_kaldi_speaker_amd import ops, _lib
    dev = torch.device("cuda:0")
    c = ops.mfcc_config()
    tables = torch.from_numpy(ops.mfcc_tables(c)).to(dev)
    pcm = torch.zeros(1000, dtype=torch.int16, device=dev)
    with pytest.raises(IndexError, match="outside"):
        ops.mfcc(c, tables, pcm, [1], [1000])
    with pytest.raises(ValueError, match="tables"):
        ops.mfcc(c, tables[:-1], pcm, [0], [1000])
    with pytest.raises(_lib.XvError, match="frame_length_ms"):
        ops.mfcc_tables(ops.mfcc_config(frame_length_ms=100.0))


def _vad_batch():
    """fp32 feature matrices of the restatement with T = 1, 2, 4, 5, 100 and 300 frames (context windows cut at both ends, one piece that
    fills the buffer), padded with rows that must not be read."""
    rs = np.random.RandomState(43)
    feats = [R.mfcc(R.signal(rs, 160 * t, 16000.0), R.VOXCELEB).astype(np.float32) for t in (1, 2, 4, 5, 100, 300)]
    assert [len(f) for f in feats] == [1, 2, 4, 5, 100, 300]
    x = np.full((len(feats), 300, 30), 1e4, np.float32)
    for i, f in enumerate(feats):
        x[i, :len(f)] = f
    return feats, x


@pytest.mark.parametrize("options", [R.VAD_VOXCELEB, VAD_SECOND], ids=["voxceleb", "no-mean-no-context"])
def test_energy_vad_equals_the_restatement(options):
    import torch
    from tf_kaldi_speaker_amd import ops
    feats, x = _vad_batch()
    ref = []
    for f in feats:
        near = float(np.abs(f[:, 0].astype(np.float64) - R.vad_threshold(f[:, 0], options["threshold"], options["mean_scale"])).min())
        assert near > 1e-2, "a frame's log-energy lies %.3g from the threshold: the decision is not determined" % near
        ref.append(R.energy_vad(f, **options))
    share = [float(m.mean()) for m in ref[-2:]]
    print("nearest / voiced share of the long pieces:", share)
    assert all(0.3 < s < 0.9 for s in share)              # both decisions occur
    dev = torch.device("cuda:0")
    rows = torch.tensor([len(f) for f in feats], dtype=torch.int32, device=dev)
    xd = torch.from_numpy(x).to(dev)
    got = ops.energy_vad(xd, rows, options["threshold"], options["mean_scale"], options["context"], options["proportion"])
    got2 = ops.energy_vad(xd, rows, options["threshold"], options["mean_scale"], options["context"], options["proportion"])
    got, got2 = got.cpu().numpy(), got2.cpu().numpy()
    assert got.dtype == np.uint8 and got.shape == (len(feats), 300) and np.array_equal(got, got2)
    for i, m in enumerate(ref):
        assert np.array_equal(got[i, :len(m)], m), (i, np.flatnonzero(got[i, :len(m)] != m))
        assert not got[i, len(m):].any(), "piece %d: mask bytes behind its rows are not zero" % i


def test_mfcc_vad_frontend_chain(cases):
    """xv_mfcc -> xv_energy_vad -> xv_frontend(cmn_window = 300, masks) on the VoxCeleb batch against restatement MFCC -> restatement VAD ->
    frontend_ref.frontend.  Masks equal (under the same 1e-2 precondition); features within the MFCC tolerance - taken at the class's
    largest |MFCC|, since CMN removes the magnitude but not the error - plus the bound of tests/test_gpu_frontend.py (2^-23 |ref| + 2^-32 A)."""
    import torch
    from tf_kaldi_speaker_amd import ops
    cfg, waves, ref64, ref32 = cases["voxceleb"]
    dev = torch.device("cuda:0")
    c = ops.mfcc_config(**cfg)
    tables = torch.from_numpy(ops.mfcc_tables(c)).to(dev)
    buf, offsets = _pack(waves)
    t = max(len(r) for r in ref64)
    x, rows = ops.mfcc(c, tables, torch.from_numpy(buf).to(dev), offsets, np.asarray([len(w) for w in waves], np.int64), t)
    masks = ops.energy_vad(x, rows)
    mask_offsets = torch.arange(len(waves), dtype=torch.int64, device=dev) * t
    out, rows_out = ops.frontend(x, rows, 300, masks.reshape(-1), mask_offsets)
    got, got_masks, rows_out = out.cpu().numpy(), masks.cpu().numpy(), rows_out.cpu().numpy()
    worst = 0.0
    for i, (r64, r32) in enumerate(zip(ref64, ref32)):
        e = r64[:, 0]
        assert float(np.abs(e - R.vad_threshold(e, 5.5, 0.5)).min()) > 1e-2
        m = R.energy_vad(r64, **R.VAD_VOXCELEB)
        assert np.array_equal(got_masks[i, :len(m)], m) and not got_masks[i, len(m):].any(), i
        y = F.frontend(r64, 300, m)
        assert rows_out[i] == len(y) and not got[i, len(y):].any(), (i, rows_out[i], len(y))
        if len(y) == 0:
            continue
        a = float(np.abs(r64).max())
        for label, cols in (("col0", slice(0, 1)), ("ceps", slice(1, 30))):
            d32 = float(np.abs(r32[:, cols].astype(np.float64) - r64[:, cols]).max())
            tol = 4.0 * d32 + 2.0 ** -21 * float(np.abs(r64[:, cols]).max()) + 2.0 ** -23 * np.abs(y[:, cols]) + 2.0 ** -32 * a
            err = np.abs(got[i, :len(y), cols].astype(np.float64) - y[:, cols])
            ratio = float((err / tol).max())
            print("chain n=%d kept %d of %d %s: max |got - ref| %.3g  worst error / tolerance %.3f" % (LENS[i], len(y), len(m), label, float(err.max()), ratio))
            worst = max(worst, ratio)
    assert worst <= 1.0, worst
    assert 0.5 < got_masks[-1, :len(ref64[-1])].mean() < 0.8      # both decisions occur on the long utterance
