"""xv_fbank on a real MI355X against the fp64 restatement (tests/fbank_ref.py, built on tests/mfcc_ref.py; Kaldi is not available: parity by
restatement), and its energy_out against xv_mfcc's column 0 and the restated VAD.

Tolerance of the features - the rule of tests/test_gpu_mfcc.py - per utterance and per column class (the log-energy column, where use_energy
puts one, apart from the mel columns): |got - ref| <= 4 * D32 + 2^-21 * |ref|, D32 the largest |fp32 restatement - fp64 restatement| over that
utterance and class: what the number format alone costs there, times 4 because the GPU's FFT order and reduction trees differ from
pocketfft's, plus two ulps for the last log (or sqrt) and the rounding.  It is measured on the restatement, never on the code under test.
The observed worst error / tolerance ratios are in profiles/fbank_parity.txt.

The four cases are the four FFT sizes, each with another bin count and another corner of the options:
  n512   16 kHz 25 / 10 ms, 23 bins, compute-fbank-feats' defaults (snip-edges, no energy column, raw energy, log, power): d = 23, odd rows
  n256    8 kHz 25 / 10 ms, 40 bins, snip-edges off, use_energy with the energy behind the window and a floor, log of MAGNITUDE sums: d = 41
  n128   16 kHz  5 /  2 ms, 65 bins (a second trip of the lane-per-bin loop; bins that hold no FFT bin), linear power sums: d = 65
  n1024  16 kHz 64 / 16 ms, 127 bins + use_energy: d = 128, the widest row; linear magnitude sums; L = N, no zero padding
Utterances per case: n < L, n = L, T = 15, 16 and 17 frames (the 16-frame walk of a workgroup: one short, exact, one over), 5003 samples,
and 0.8 s with a quiet stretch (both VAD decisions)."""
import numpy as np
import pytest

from tests import fbank_ref as FB
from tests import mfcc_ref as R

pytestmark = pytest.mark.gpu

CASES = {
    "n512": FB.config(),
    "n256": FB.config(sample_frequency=8000.0, num_mel_bins=40, high_freq=3700.0, snip_edges=0, use_energy=1, raw_energy=0, energy_floor=3.0e5,
                      use_power=0),
    "n128": FB.config(frame_length_ms=5.0, frame_shift_ms=2.0, num_mel_bins=65, high_freq=7600.0, use_log_fbank=0),
    "n1024": FB.config(frame_length_ms=64.0, frame_shift_ms=16.0, num_mel_bins=127, use_energy=1, use_log_fbank=0, use_power=0),
}
VAD = dict(R.VAD_VOXCELEB)


def _lens(cfg):
    L, S, _ = FB.dims(cfg)
    frames = (lambda t: L + (t - 1) * S) if cfg["snip_edges"] else (lambda t: t * S - S // 2)
    lens = [L - 1, L, frames(15), frames(16), frames(17), 5003, int(0.8 * cfg["sample_frequency"])]
    assert [FB.num_frames(n, cfg) for n in lens[2:5]] == [15, 16, 17]
    return lens


@pytest.fixture(scope="module")
def cases():
    """Per case: the waveforms, the fp64 and fp32 restatements of the features and of logE; computed once, read only."""
    out = {}
    for name, cfg in CASES.items():
        assert FB.dims(cfg)[2] == int(name[1:])
        rs = np.random.RandomState(71)
        lens = _lens(cfg)
        waves = [R.signal(rs, n, cfg["sample_frequency"]) for n in lens]
        ref64 = [FB.fbank(w, cfg, np.float64, with_energy=True) for w in waves]
        ref32 = [FB.fbank(w, cfg, np.float32, with_energy=True) for w in waves]
        for a in waves + [x for pair in ref64 + ref32 for x in pair]:
            a.setflags(write=False)
        out[name] = (cfg, lens, waves, ref64, ref32)
    return out


def _pack(waves):
    """Back to back behind one stray sample: odd and even offsets, no alignment beyond two bytes."""
    offsets = 1 + np.concatenate([[0], np.cumsum([len(w) for w in waves])[:-1]]).astype(np.int64)
    return np.concatenate([np.array([12345], np.int16)] + list(waves)), offsets


def _run(cfg, waves, t_out, with_energy=True):
    """Two calls on the same input; their bits must agree.  -> (features, rows, energy [b, t_out]) as host arrays."""
    import torch
    from tf_kaldi_speaker_amd import ops
    dev = torch.device("cuda:0")
    c = ops.fbank_config(**cfg)
    tables = torch.from_numpy(ops.fbank_tables(c)).to(dev)
    buf, offsets = _pack(waves)
    pcm = torch.from_numpy(buf).to(dev)
    lens = np.asarray([len(w) for w in waves], np.int64)
    a = ops.fbank(c, tables, pcm, offsets, lens, t_out, with_energy=with_energy)
    b = ops.fbank(c, tables, pcm, offsets, lens, t_out, with_energy=with_energy)
    torch.cuda.synchronize()
    host = [[None if t is None else t.cpu().numpy() for t in call] for call in (a, b)]
    for x, y in zip(*host):
        assert (x is None and y is None) or np.array_equal(x.view(np.uint32), y.view(np.uint32)), "two calls on the same input differ"
    out, rows, energy = host[0]
    assert energy is None or energy.shape == (len(waves), t_out, 1)
    return out, rows, None if energy is None else energy[:, :, 0]


def _ratio(got, r64, r32):
    d32 = float(np.abs(r32.astype(np.float64) - r64).max())
    tol = 4.0 * d32 + 2.0 ** -21 * np.abs(r64)
    err = np.abs(got.astype(np.float64) - r64)
    return d32, float(err.max()), float((err / tol).max())


@pytest.mark.parametrize("name", sorted(CASES))
def test_fbank_against_the_restatement(cases, name):
    cfg, lens, waves, ref64, ref32 = cases[name]
    d, ue = FB.width(cfg), cfg["use_energy"]
    t_out = max(len(f) for f, _ in ref64)
    assert (d % 2 == 1) == (name != "n1024") and (d == 128) == (name == "n1024")
    assert (FB.tables(cfg)["mel_count"].min() == 0) == (name == "n128")      # 8 of its 65 bins hold no FFT bin: E = 0 there
    got, rows, energy = _run(cfg, waves, t_out)
    assert got.shape == (len(lens), t_out, d)
    worst = 0.0
    for i, ((f64, e64), (f32, e32)) in enumerate(zip(ref64, ref32)):
        keep = len(f64)
        assert rows[i] == keep == FB.num_frames(lens[i], cfg), (i, rows[i], keep)
        assert not got[i, keep:].any() and not energy[i, keep:].any(), "utterance %d: rows behind rows_out are not exactly zero" % i
        if keep == 0:
            continue
        assert np.isfinite(got[i, :keep]).all()
        classes = [("mel", got[i, :keep, ue:], f64[:, ue:], f32[:, ue:]), ("energy_out", energy[i, :keep], e64, e32)]
        if ue:
            classes.append(("col0", got[i, :keep, 0], f64[:, 0], f32[:, 0]))
            assert np.array_equal(got[i, :keep, 0].view(np.uint32), energy[i, :keep].view(np.uint32)), "column 0 is energy_out"
        for label, g, r64, r32 in classes:
            d32, err, ratio = _ratio(g, r64, r32)
            print("%s n=%d T=%d %s: D32 %.3g  max |got - ref| %.3g  max |ref| %.4g  worst error / tolerance %.3f"
                  % (name, lens[i], keep, label, d32, err, float(np.abs(r64).max()), ratio))
            worst = max(worst, ratio)
    print("%s: worst error / tolerance %.3f" % (name, worst))
    assert worst <= 1.0, worst
    # t_out below most frame counts: the output is cut, rows_out says so, a frame's bits do not depend on t_out; and without energy_out
    cut, rows_cut, none = _run(cfg, waves, 7, with_energy=False)
    assert none is None and np.array_equal(rows_cut, np.minimum(rows, 7))
    assert np.array_equal(cut.view(np.uint32), got[:, :7].view(np.uint32))


@pytest.mark.parametrize("name", sorted(CASES))
def test_an_utterance_alone_and_as_the_third_of_five_give_the_same_bits(cases, name):
    cfg, lens, waves, ref64, _ = cases[name]
    t_out = max(len(f) for f, _ in ref64)
    five = [waves[3], waves[1], waves[6], waves[0], waves[5]]
    a, rows_a, e_a = _run(cfg, five, t_out)
    b, rows_b, e_b = _run(cfg, [waves[6]], t_out)
    assert rows_a[2] == rows_b[0] == len(ref64[6][0]) > 16
    assert np.array_equal(a[2].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(e_a[2].view(np.uint32), e_b[0].view(np.uint32))


@pytest.mark.parametrize("name", sorted(CASES))
def test_energy_out_is_column_0_of_xv_mfcc_and_gives_its_mask(cases, name):
    """With the options of an xv_mfcc_config (use_energy on) energy_out holds the bits of that call's column 0 - whatever the fbank call's
    own use_energy, use_log_fbank and use_power say - so the masks of xv_energy_vad agree; and they equal the restated mask, after the
    test has shown ON THE REFERENCE that every frame's logE lies further than 100 * D32 from the threshold (no frame is left out)."""
    import torch
    from tf_kaldi_speaker_amd import ops
    cfg, lens, waves, ref64, ref32 = cases[name]
    dev = torch.device("cuda:0")
    t_out = max(len(f) for f, _ in ref64)
    buf, offsets = _pack(waves)
    pcm = torch.from_numpy(buf).to(dev)
    n = np.asarray(lens, np.int64)
    fc = ops.fbank_config(**cfg)
    _, rows_f, energy = ops.fbank(fc, torch.from_numpy(ops.fbank_tables(fc)).to(dev), pcm, offsets, n, t_out)
    mc = ops.mfcc_config(**FB.as_mfcc(cfg, use_energy=1, num_ceps=min(13, cfg["num_mel_bins"]), cepstral_lifter=22.0))
    x, rows_m = ops.mfcc(mc, torch.from_numpy(ops.mfcc_tables(mc)).to(dev), pcm, offsets, n, t_out)
    assert torch.equal(rows_f, rows_m)
    assert np.array_equal(energy.cpu().numpy()[:, :, 0].view(np.uint32), x.cpu().numpy()[:, :, 0].view(np.uint32))
    args = (VAD["threshold"], VAD["mean_scale"], VAD["context"], VAD["proportion"])
    mask_f, mask_m = ops.energy_vad(energy, rows_f, *args).cpu().numpy(), ops.energy_vad(x, rows_m, *args).cpu().numpy()
    assert np.array_equal(mask_f, mask_m)
    decisions = set()
    for i, ((_, e64), (_, e32)) in enumerate(zip(ref64, ref32)):
        if len(e64) == 0:
            assert not mask_f[i].any()
            continue
        d32 = float(np.abs(e32.astype(np.float64) - e64).max())
        near = float(np.abs(e64 - R.vad_threshold(e64, VAD["threshold"], VAD["mean_scale"])).min())
        print("%s n=%d: D32 of logE %.3g, the nearest frame lies %.3g from the threshold" % (name, lens[i], d32, near))
        assert near > 100.0 * d32, "a frame's log-energy lies %.3g from the threshold (100 D32 = %.3g): the decision is not determined" % (near, 100.0 * d32)
        want = R.energy_vad(e64[:, None], **VAD)
        assert np.array_equal(mask_f[i, :len(want)], want) and not mask_f[i, len(want):].any(), (i, np.flatnonzero(mask_f[i, :len(want)] != want))
        decisions |= set(want.tolist())
    assert decisions == {0, 1}                                                 # both decisions occur (the 0.8 s utterance has a quiet stretch)


def test_fbank_refuses_bad_arguments_without_a_launch():
    import ctypes as C
    import torch
    from tf_kaldi_speaker_amd import _lib, ops
    dev = torch.device("cuda:0")
    c = ops.fbank_config()
    tables = torch.from_numpy(ops.fbank_tables(c)).to(dev)
    pcm = torch.zeros(1000, dtype=torch.int16, device=dev)
    with pytest.raises(IndexError, match="fbank: .*outside"):
        ops.fbank(c, tables, pcm, [1], [1000])
    with pytest.raises(ValueError, match="fbank: tables"):
        ops.fbank(c, tables[:-1], pcm, [0], [1000])
    with pytest.raises(ValueError, match="fbank: tables"):                      # xv_mfcc's tables are longer by the dct block
        ops.fbank(c, torch.from_numpy(ops.mfcc_tables(ops.mfcc_config())).to(dev), pcm, [0], [1000])
    with pytest.raises(ValueError, match="fbank: pcm"):
        ops.fbank(c, tables, pcm.to(torch.int32), [0], [1000])
    with pytest.raises(ValueError, match="one length"):
        ops.fbank(c, tables, pcm, [0, 10], [1000])
    with pytest.raises(_lib.XvError, match="129 columns"):
        wide = ops.fbank_config(num_mel_bins=128, use_energy=1)
        ops.fbank(wide, tables, pcm, [0], [1000])
    with pytest.raises(_lib.XvError, match="frame_length_ms"):
        ops.fbank_tables(ops.fbank_config(frame_length_ms=100.0))
    # the entry point itself: null pointers, no utterance, no row - refused before anything is launched (the output keeps its bytes)
    lib = _lib.load()
    out = torch.full((1, 4, 23), 7.0, device=dev)
    rows = torch.full((1,), -5, dtype=torch.int32, device=dev)
    off, n = torch.zeros(1, dtype=torch.int64, device=dev), torch.full((1,), 1000, dtype=torch.int32, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    for b, t_out, tb in ((0, 4, p(tables)), (1, 0, p(tables)), (1, 4, C.c_void_p(0)), (70000, 4, p(tables))):
        assert lib.xv_fbank(None, C.byref(c), tb, p(pcm), p(off), p(n), b, t_out, p(out), p(rows), None) == 2
        assert lib.xv_last_error().decode().startswith("fbank:")
    torch.cuda.synchronize()
    assert float(out.min()) == 7.0 and int(rows[0]) == -5
