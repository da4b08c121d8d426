"""xv_resample on a real MI355X against the fp64 restatement (tests/resample_ref.py; Kaldi is not available: parity by restatement).

Tolerance on out_f32, per sample: |got - ref64| <= 4 * D32 + 2^-21 * |ref64|, D32 the largest |fp32 restatement - fp64 restatement| over
that utterance: what the number format alone costs, measured on the restatement, never on the kernel (tests/test_gpu_augment.py).  The
derived bound is asserted beside it: (taps_max + 1) * 2^-24 * sum_j |w| |x| + 2^-21 |ref64| - one rounding per fma of the chain and one
for the weights' own rounding to fp32, each relative to the sum of magnitudes that reached the sample.  Shapes come from
xv_debug_resample_plan (the tile, taps_max, the units), not from constants copied here.  out_pcm and the clip counts are held EXACTLY
against rint-then-clamp of the kernel's own out_f32; the main cases clip nothing in the fp64 restatement (asserted on the reference first).
The worst ratios of each pair are printed (profiles/resample_parity.txt records a run)."""
import numpy as np
import pytest

from tests import resample_ref as R

pytestmark = pytest.mark.gpu

PCM_FILL, F32_FILL = 23130, -7777.25


def _pack(arrays):
    """Back to back behind one stray sample: odd first offset, no alignment beyond two bytes (tests/test_gpu_mfcc.py: _pack)."""
    offsets = 1 + np.concatenate([[0], np.cumsum([len(a) for a in arrays])[:-1]]).astype(np.int64)
    return np.concatenate([np.array([12345], np.int16)] + [np.asarray(a, np.int16) for a in arrays]), offsets


def _call(cfg, utts, gap=3):
    """One ops.resample call -> per utterance (out_f32, out_pcm, clipped), after the checks every call gets: out_samples as the closed form,
    the samples between the utterances untouched, two calls bit-identical."""
    import torch
    from tf_kaldi_speaker_amd import ops
    dev = torch.device("cuda:0")
    tables = torch.from_numpy(ops.resample_tables(cfg)).to(dev)
    src, src_off = _pack(utts)
    n_out = np.asarray([ops.resample_num_samples(cfg, len(x)) for x in utts], np.int64)
    out_off = 1 + np.concatenate([[0], np.cumsum(n_out + gap)[:-1]]).astype(np.int64)
    total = int(out_off[-1] + n_out[-1] + gap)
    src_d = torch.from_numpy(src).to(dev)
    runs = []
    for _ in range(2):
        pcm = torch.full((total,), PCM_FILL, dtype=torch.int16, device=dev)
        f32 = torch.full((total,), F32_FILL, dtype=torch.float32, device=dev)
        _, off, samples, clipped, _ = ops.resample(cfg, tables, src_d, src_off, [len(x) for x in utts], out_offsets=out_off, out_pcm=pcm, out_f32=f32)
        torch.cuda.synchronize()
        runs.append((pcm.cpu().numpy(), f32.cpu().numpy(), samples.cpu().numpy(), clipped.cpu().numpy()))
        assert np.array_equal(off, out_off)
    (pcm, f32, samples, clipped), again = runs
    assert np.array_equal(pcm, again[0]) and np.array_equal(f32.view(np.uint32), again[1].view(np.uint32)), "two calls on the same input differ"
    assert np.array_equal(samples, again[2]) and np.array_equal(clipped, again[3])
    assert np.array_equal(samples, n_out)
    written = np.zeros(total, bool)
    for o, m in zip(out_off, n_out):
        written[o:o + m] = True
    assert (pcm[~written] == PCM_FILL).all() and (f32[~written] == np.float32(F32_FILL)).all(), "samples between the utterances were written"
    assert np.isfinite(f32[written]).all()
    return [(f32[o:o + m], pcm[o:o + m], int(c)) for o, m, c in zip(out_off, n_out, clipped)]


def _quantiser_is_exact(f32, pcm, clipped, where):
    want, count = R.quantise(f32)      # rint-then-clamp of the kernel's OWN fp32 values
    assert np.array_equal(pcm, want) and clipped == count, where


def _pair(fin, fout):
    from tf_kaldi_speaker_amd import ops
    cfg = ops.resample_config(fin, fout)
    hook = ops.resample_plan(cfg)
    plan = R.Plan(fin, fout)
    assert (hook["in_unit"], hook["out_unit"], hook["taps_max"]) == (plan.in_unit, plan.out_unit, plan.taps_max)
    tile = hook["tile"]
    # an utterance across three tiles with a remainder of 7 outputs in the last (8 where the pair only gives even lengths)
    n3 = next(n for n in range(1, 4 * tile * plan.in_unit) if plan.num_samples(n) >= 2 * tile + 7)
    assert 7 <= plan.num_samples(n3) - 2 * tile <= 8
    lengths = [1, 2, plan.taps_max - 1, plan.in_unit, plan.in_unit + 1, 1023, 1024, 1025, 2051, n3]
    rs = np.random.RandomState(fin % 9973 + fout)
    utts = [R.signal(rs, n, float(fin)) for n in lengths]
    got = _call(cfg, utts)
    worst = [0.0, 0.0, 0.0]
    for i, (x, (f32, pcm, clipped)) in enumerate(zip(utts, got)):
        where = "%d -> %d, utterance %d (%d samples)" % (fin, fout, i, len(x))
        d = {}
        r64 = R.resample(x, plan, np.float64, details=d)
        r32 = R.resample(x, plan, np.float32)
        assert R.quantise(r64)[1] == 0 and np.abs(r64).max() < 32000, "%s: the reference clips; the case is ill chosen" % where
        assert f32.shape == r64.shape == (plan.num_samples(len(x)),)
        d32 = float(np.abs(r32.astype(np.float64) - r64).max())
        err = np.abs(f32.astype(np.float64) - r64)
        tol = 4.0 * d32 + 2.0 ** -21 * np.abs(r64)
        bound = (plan.taps_max + 1) * 2.0 ** -24 * d["magnitude"] + 2.0 ** -21 * np.abs(r64)
        ref_ratio = float((np.abs(r32.astype(np.float64) - r64) / np.maximum(bound, 1e-30)).max())
        ratios = (float((err / np.maximum(tol, 1e-30)).max()), float((err / np.maximum(bound, 1e-30)).max()))
        worst = [max(worst[0], ratios[0]), max(worst[1], ratios[1]), max(worst[2], ref_ratio)]
        assert (err <= tol).all(), "%s: %.3g of the tolerance" % (where, ratios[0])
        assert (err <= bound).all(), "%s: %.3g of the derived bound" % (where, ratios[1])
        _quantiser_is_exact(f32, pcm, clipped, where)
        assert clipped == 0
    print("PARITY %d -> %d: %d utterances, tile %d, taps_max %d: worst |got - ref64| = %.3f of the tolerance, %.3f of the derived bound "
          "(the fp32 restatement: %.3f of the derived bound)" % (fin, fout, len(utts), tile, plan.taps_max, worst[0], worst[1], worst[2]))
    # an utterance alone and as the third of five: the same bits
    alone = _call(cfg, [utts[8]])[0]
    third = _call(cfg, [utts[5], utts[9], utts[8], utts[0], utts[6]])[2]
    assert np.array_equal(alone[0].view(np.uint32), third[0].view(np.uint32)) and np.array_equal(alone[1], third[1])
    assert np.array_equal(alone[0].view(np.uint32), got[8][0].view(np.uint32))


def test_16000_to_8000_one_phase():
    _pair(16000, 8000)


def test_8000_to_16000_two_phases_upsampling():
    _pair(8000, 16000)


def test_14400_to_16000_speed_0_9():
    _pair(14400, 16000)


def test_17600_to_16000_speed_1_1():
    _pair(17600, 16000)


def test_44100_to_16000_160_phases():
    _pair(44100, 16000)


def test_16000_to_11025_the_largest_table():
    _pair(16000, 11025)


def test_a_full_scale_constant_clips_in_the_interior():
    """Row sum 1.00046 of 16000 -> 8000: 32767 becomes 32782 in the fp64 restatement; the counts equal the restatement's."""
    from tf_kaldi_speaker_amd import ops
    cfg = ops.resample_config(16000, 8000)
    plan = R.Plan(16000, 8000)
    utts = [np.full(2 * ops.resample_plan(cfg)["tile"] * 2 + 10, 32767, np.int16), np.full(300, -32768, np.int16), R.signal(np.random.RandomState(3), 500)]
    got = _call(cfg, utts)
    for i, (x, (f32, pcm, clipped)) in enumerate(zip(utts, got)):
        r64 = R.resample(x, plan)
        want_pcm, want_clipped = R.quantise(r64)
        _quantiser_is_exact(f32, pcm, clipped, "utterance %d" % i)
        assert clipped == want_clipped and np.abs(pcm.astype(np.int64) - want_pcm).max() <= 1, (i, clipped, want_clipped)
    assert round(float(R.resample(utts[0], plan)[100])) == 32782 and got[0][2] > 1900 and got[0][1][100] == 32767 and got[2][2] == 0


def test_bad_arguments_are_refused_before_any_launch():
    import torch
    from tf_kaldi_speaker_amd import _lib, ops
    dev = torch.device("cuda:0")
    cfg = ops.resample_config(16000, 8000)
    tables = torch.from_numpy(ops.resample_tables(cfg)).to(dev)
    pcm = torch.zeros(1000, dtype=torch.int16, device=dev)
    with pytest.raises(IndexError, match="lies outside the 1000 samples"):
        ops.resample(cfg, tables, pcm, [900], [101])
    with pytest.raises(IndexError, match="lies outside"):
        ops.resample(cfg, tables, pcm, [-1], [10])
    with pytest.raises(ValueError, match="tables must be resample_tables"):
        ops.resample(cfg, tables[:-1], pcm, [0], [10])
    with pytest.raises(ValueError, match="tables must be resample_tables"):
        ops.resample(ops.resample_config(16000, 11025), tables, pcm, [0], [10])
    with pytest.raises(ValueError, match="one length"):
        ops.resample(cfg, tables, pcm, [0, 10], [10])
    with pytest.raises(IndexError, match="overlap or lie outside"):
        ops.resample(cfg, tables, pcm, [0, 100], [100, 100], out_offsets=[0, 49])
    with pytest.raises(IndexError, match="overlap or lie outside"):
        ops.resample(cfg, tables, pcm, [0], [100], out_pcm=torch.zeros(49, dtype=torch.int16, device=dev))
    with pytest.raises(ValueError, match="int16"):
        ops.resample(cfg, tables, pcm.float(), [0], [10])
    with pytest.raises(_lib.XvError, match="nothing to resample"):
        ops.resample(ops.resample_config(8000, 8000), tables, pcm, [0], [10])
    with pytest.raises(_lib.XvError, match="more than 16384"):
        ops.resample(ops.resample_config(16000, 15999), tables, pcm, [0], [10])
    out, off, samples, clipped, f32 = ops.resample(cfg, tables, pcm, [0, 500], [0, 11])      # an empty utterance gives no output
    assert samples.cpu().tolist() == [0, 6] and off.tolist() == [0, 0] and f32 is None and clipped.cpu().tolist() == [0, 0]
