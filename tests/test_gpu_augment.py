"""xv_augment on a real MI355X against the fp64 restatement (tests/augment_ref.py; Kaldi is not available: parity by restatement).

Tolerance on out_f32, per sample: |got - ref64| <= 4 * D32 + 2^-21 * |ref64|, D32 the largest |fp32 restatement - fp64 restatement| over
that utterance with the kernels' block size (from the plan hook): what the number format alone costs, measured on the restatement, never
on the kernel, times 4 for a different add order (tests/test_gpu_mfcc.py).  The derived bound is asserted beside it:
(chain(L) + J + 2) * 2^-24 * s * (|x| * |h| + sum g_j |v_j|) + 2^-21 |ref| - chain(L) roundings of the convolution, one per noise, one for
the scale and one for the scale's own rounding, each relative to the sum of magnitudes that reached the sample.  The fp32 restatement sits
at <= 0.25 of the derived bound on these shapes (0.01 under 4 001 taps; printed per utterance), so the D32 form binds.  (The 0.25 belongs to
the utterances without an impulse response: there chain(L) = 0 and the bound is only J + 2 roundings, of which the J + 1 of the additions and the
scale really occur, each at most 2^-24 relative and seldom all at their worst in one sample; under an impulse response the bound counts chain(L) >= 33 roundings in the worst case while
the errors of a blocked sum add like a random walk, hence 0.01 - 0.1.)  Shapes come from xv_debug_augment_plan (T = XV_AUG_TILE, KB =
XV_AUG_KB), not from constants copied here.  out_pcm and the clip counts are held EXACTLY against truncate-and-clamp of the kernel's own
out_f32; the main cases clip nothing in the fp64 restatement (asserted on the reference first)."""
import numpy as np
import pytest

from tests import augment_ref as A

pytestmark = pytest.mark.gpu

SNRS = (15.0, 10.0, 5.0, 0.0, 20.0, 17.0, 13.0, 8.0)
PCM_FILL, F32_FILL = 23130, -7777.25
CONVOLUTIONS = {}      # the restatement's convolutions, shared by the configurations that run the same utterances


@pytest.fixture(scope="module")
def hook():
    from tf_kaldi_speaker_amd import ops
    p = ops.augment_plan(1)
    return p["tile"], p["kb"]


def _pack(arrays):
    """Back to back behind one stray sample: odd first offset, no alignment beyond two bytes (tests/test_gpu_mfcc.py: _pack)."""
    offsets = 1 + np.concatenate([[0], np.cumsum([len(a) for a in arrays])[:-1]]).astype(np.int64)
    return np.concatenate([np.array([12345], np.int16)] + [np.asarray(a, np.int16) for a in arrays]), offsets


def _noises(rs, kind, M, T, pool):
    """J = 0 | one foreground noise that starts in the last tile | one background | three mixed, one of them starting at o >= M."""
    last = min((M - 1) // T * T + 3, M - 1)
    snr = lambda: SNRS[rs.randint(len(SNRS))]
    if kind == 0:
        return []
    if kind == 1:
        return [(pool[0], snr(), last, None)]
    if kind == 2:
        return [(pool[1], snr(), 0, "bg")]
    return [(pool[2], snr(), min(3, M - 1), None), (pool[1], snr(), 0, "bg"), (pool[0], snr(), M + 5, None)]


def _call(cfg_kw, utts, gap=3):
    """One ops.augment call over utts = [(x, h | None, noises)] -> per utterance (out_f32, out_pcm, clipped), after the checks every call
    gets: out_samples / offsets as step 6 says, the samples between the utterances untouched, two calls bit-identical."""
    import torch
    from tf_kaldi_speaker_amd import ops
    dev = torch.device("cuda:0")
    cfg = ops.augment_config(**cfg_kw)
    src, src_off = _pack([u[0] for u in utts])
    rirs, rir_ids, noises, noise_ids = [], {}, [], {}
    utt_rir, first, nz = [], [0], []
    for x, h, ns in utts:
        if h is not None and id(h) not in rir_ids:
            rir_ids[id(h)] = len(rirs)
            rirs.append(h)
        utt_rir.append(-1 if h is None else rir_ids[id(h)])
        for v, snr, start, span in ns:
            if id(v) not in noise_ids:
                noise_ids[id(v)] = len(noises)
                noises.append(v)
            nz.append((noise_ids[id(v)], snr, start, len(v) if span is None else -1 if span == "bg" else span))
        first.append(len(nz))
    M = [len(x) + (len(h) - 1 if h is not None else 0) for x, h, _ in utts]
    n_out = np.asarray([len(u[0]) if cfg.shift_output else m for u, m in zip(utts, M)], np.int64)
    out_off = 1 + np.concatenate([[0], np.cumsum(n_out + gap)[:-1]]).astype(np.int64)
    total = int(out_off[-1] + n_out[-1] + gap)
    kw = dict(nz_first=first)
    if rirs:
        rir, rir_off = _pack(rirs)
        kw.update(rir=torch.from_numpy(rir).to(dev), rir_off=rir_off, rir_len=[len(h) for h in rirs],
                  rir_early=[ops.augment_early(h, cfg.sample_frequency) for h in rirs], utt_rir=utt_rir)
        assert kw["rir_early"] == [A.early(h, cfg.sample_frequency) for h in rirs]
    if nz:
        noise, noise_off = _pack(noises)
        kw.update(noise=torch.from_numpy(noise).to(dev), noise_off=noise_off, noise_len=[len(v) for v in noises], nz_id=[e[0] for e in nz],
                  nz_snr=[e[1] for e in nz], nz_start=[e[2] for e in nz], nz_span=[e[3] for e in nz])
    src_d = torch.from_numpy(src).to(dev)
    runs = []
    for _ in range(2):
        pcm = torch.full((total,), PCM_FILL, dtype=torch.int16, device=dev)
        f32 = torch.full((total,), F32_FILL, dtype=torch.float32, device=dev)
        _, off, samples, clipped, _ = ops.augment(cfg, src_d, src_off, [len(u[0]) for u in utts], out_offsets=out_off, out_pcm=pcm, out_f32=f32, **kw)
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


def _check(label, cfg_kw, utts, got, kb, clips=False):
    """The two bounds on out_f32 and the exact quantiser rule, per utterance -> the worst ratios of this call."""
    from tf_kaldi_speaker_amd import ops
    worst = [0.0, 0.0]
    for i, ((x, h, ns), (f32, pcm, clipped)) in enumerate(zip(utts, got)):
        d = {}
        r64 = A.augment(x, h, ns, dtype=np.float64, details=d, cache=CONVOLUTIONS, **cfg_kw)
        r32 = A.augment(x, h, ns, dtype=np.float32, kb=kb, cache=CONVOLUTIONS, **cfg_kw)
        if not clips:
            assert A.quantise(r64)[1] == 0 and np.abs(r64).max() < 32000, "%s %d: the reference clips; the case is ill chosen" % (label, i)
        assert f32.shape == r64.shape
        d32 = float(np.abs(r32.astype(np.float64) - r64).max())
        chain = ops.augment_plan(len(x), len(h))["chain"] if h is not None else 0
        assert chain == (kb + -(-len(h) // kb) if h is not None else 0)
        err = np.abs(f32.astype(np.float64) - r64)
        tol = 4.0 * d32 + 2.0 ** -21 * np.abs(r64)
        derived = (chain + len(ns) + 2) * 2.0 ** -24 * d["scale"] * d["magnitude"] + 2.0 ** -21 * np.abs(r64)
        ratios = [float((err / np.maximum(t, 1e-300)).max()) if err.max() > 0 else 0.0 for t in (tol, derived)]
        print("%s n=%d L=%d p=%d J=%d: D32 %.3g  max |got - ref| %.3g  max |ref| %.5g  error / tolerance %.3f  error / derived bound %.4f  "
              "fp32 restatement / derived bound %.4f" % (label, len(x), 0 if h is None else len(h), d["p"], len(ns), d32, float(err.max()),
                                                        float(np.abs(r64).max()), ratios[0], ratios[1],
                                                        float((np.abs(r32 - r64) / np.maximum(derived, 1e-300)).max())))
        assert ratios[0] <= 1.0 and ratios[1] <= 1.0, (label, i, ratios)
        q, count = A.quantise(f32)
        assert np.array_equal(pcm, q) and clipped == count, (label, i, clipped, count)
        worst = [max(a, b) for a, b in zip(worst, ratios)]
    print("%s: worst error / tolerance %.3f, worst error / derived bound %.4f over %d utterances" % (label, worst[0], worst[1], len(utts)))
    return worst


def _grid(hook, rs):
    """n in {1, T - 1, T, T + 1, 2 T + 3} x L in {1, KB - 1, KB, KB + 1, 3 KB + 5, n + 7 (> n)} x peak in {0, 37, L - 1}; the noise lists
    cycle through the four forms."""
    T, KB = hook
    pool = [A.signal(rs, 50), A.signal(rs, 301), A.signal(rs, 700)]
    utts, seen = [], 0
    for n in (1, T - 1, T, T + 1, 2 * T + 3):
        x = A.signal(rs, n)
        for L in (1, KB - 1, KB, KB + 1, 3 * KB + 5, n + 7):
            for peak in sorted({0, min(37, L - 1), L - 1}):
                utts.append((x, A.rir(rs, L, peak), _noises(rs, seen % 4, n + L - 1, T, pool)))
                seen += 1
    return utts


@pytest.mark.parametrize("cfg_kw", [dict(shift_output=1, normalize_output=1, volume=0.0), dict(shift_output=0, normalize_output=1, volume=0.5)],
                         ids=["shift-normalize", "full-normalize-volume"])
def test_reverberation_grid(hook, cfg_kw):
    utts = _grid(hook, np.random.RandomState(61))
    assert len(utts) >= 60 and {len(u[2]) for u in utts} == {0, 1, 3}
    _check("grid " + "/".join("%s=%g" % kv for kv in sorted(cfg_kw.items())), cfg_kw, utts, _call(cfg_kw, utts), hook[1])


@pytest.mark.parametrize("cfg_kw", [dict(shift_output=1, normalize_output=0, volume=0.0), dict(shift_output=0, normalize_output=0, volume=0.5),
                                    dict(shift_output=1, normalize_output=1, volume=0.0)],
                         ids=["plain", "volume", "normalize"])
def test_noise_without_impulse_response(hook, cfg_kw):
    T, KB = hook
    rs = np.random.RandomState(67)
    pool = [A.signal(rs, 50), A.signal(rs, 301), A.signal(rs, 700)]
    utts = [(A.signal(rs, n), None, _noises(rs, kind, n, T, pool)) for n in (1, T - 1, T, T + 1, 2 * T + 3) for kind in range(4)]
    got = _call(cfg_kw, utts)
    _check("no-rir " + "/".join("%s=%g" % kv for kv in sorted(cfg_kw.items())), cfg_kw, utts, got, KB)
    if not cfg_kw["normalize_output"] and not cfg_kw["volume"]:
        for (x, _, ns), (f32, pcm, _) in zip(utts, got):
            if not ns:
                assert np.array_equal(pcm, x) and np.array_equal(f32, x.astype(np.float32))      # nothing to do: the source itself


def test_biggest_case_and_batch_independence(hook):
    """About 9 000 samples under 4 001 taps with three noises (several chunks of taps, several tiles, chunks that are skipped), alone and as
    the third of a batch of five: an utterance's bits do not depend on what else is in the batch."""
    T, KB = hook
    rs = np.random.RandomState(71)
    pool = [A.signal(rs, 50), A.signal(rs, 301), A.signal(rs, 700)]
    cfg_kw = dict(shift_output=1, normalize_output=1, volume=0.0)
    x, h = A.signal(rs, 9001), A.rir(rs, 4001, 37)
    big = (x, h, _noises(rs, 3, 9001 + 4000, T, pool))
    alone = _call(cfg_kw, [big])
    _check("biggest", cfg_kw, [big], alone, KB)
    others = [(A.signal(rs, T + 1), A.rir(rs, KB + 1, 0), []), (A.signal(rs, 700), None, _noises(rs, 2, 700, T, pool)),
              (A.signal(rs, 3 * T), h, _noises(rs, 1, 3 * T + 4000, T, pool)), (A.signal(rs, 1), None, [])]
    batch = others[:2] + [big] + others[2:]
    got = _call(cfg_kw, batch)
    assert np.array_equal(got[2][0].view(np.uint32), alone[0][0].view(np.uint32)) and np.array_equal(got[2][1], alone[0][1])
    assert got[2][2] == alone[0][2]
    _check("batch of five", cfg_kw, others, got[:2] + got[3:], KB)


def test_clipping_is_truncate_then_clamp_and_counted(hook):
    """volume = 6 (and an impulse response without normalisation, whose output is far outside PCM-16) clip on purpose: out_pcm is the exact
    quantiser of out_f32 and `clipped` its count."""
    T, KB = hook
    rs = np.random.RandomState(73)
    utts = [(A.signal(rs, 2 * T + 3), A.rir(rs, 3 * KB + 5, 37), []), (A.signal(rs, T - 1), None, [(A.signal(rs, 301), 5.0, 0, "bg")])]
    for cfg_kw in (dict(shift_output=1, normalize_output=1, volume=6.0), dict(shift_output=0, normalize_output=0, volume=0.0)):
        got = _call(cfg_kw, utts)
        _check("clipping " + "/".join("%s=%g" % kv for kv in sorted(cfg_kw.items())), cfg_kw, utts, got, KB, clips=True)
        assert sum(c for _, _, c in got) > 0, "nothing clipped: the case is ill chosen"
        for f32, pcm, clipped in got:
            assert clipped == int((f32 >= 32768.0).sum() + (f32 <= -32769.0).sum())
            if clipped:
                assert pcm.max() == 32767 or pcm.min() == -32768
            assert not pcm[np.abs(f32) < 1.0].any()                      # |v| < 1 truncates to 0, whatever its sign


def test_augment_refuses_bad_arguments():
    import torch
    from tf_kaldi_speaker_amd import ops
    dev = torch.device("cuda:0")
    cfg = ops.augment_config()
    src = torch.zeros(1000, dtype=torch.int16, device=dev)
    rir = torch.ones(100, dtype=torch.int16, device=dev)
    with pytest.raises(IndexError, match="outside"):
        ops.augment(cfg, src, [1], [1000])
    with pytest.raises(IndexError, match="empty"):
        ops.augment(cfg, src, [0], [0])
    with pytest.raises(IndexError, match="impulse response"):
        ops.augment(cfg, src, [0], [1000], rir=rir, rir_off=[1], rir_len=[100], rir_early=[(0, 100, 0)], utt_rir=[0])
    with pytest.raises(ValueError, match="es < ee"):
        ops.augment(cfg, src, [0], [1000], rir=rir, rir_off=[0], rir_len=[100], rir_early=[(5, 5, 0)], utt_rir=[0])
    with pytest.raises(IndexError, match="names a noise"):
        ops.augment(cfg, src, [0], [1000], noise=rir, noise_off=[0], noise_len=[100], nz_first=[0, 1], nz_id=[1], nz_snr=[10.0], nz_start=[0], nz_span=[100])
    with pytest.raises(IndexError, match="overlap"):
        ops.augment(cfg, src, [0, 0], [1000, 1000], out_offsets=[0, 999])
