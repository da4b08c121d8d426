"""The host side of the augmentation stage (misc/augment.py) and the two host-only entry points of its C-ABI family: the plan parser and
its refusals, the seeded plan generator, the option table, the wav writer, xv_debug_augment_plan and xv_augment_workspace_bytes.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from tf_kaldi_speaker_amd.misc import augment, features


def _plan(tmp_path, text):
    path = tmp_path / "plan"
    path.write_text(text)
    return str(path)


def test_plan_parser_reads_good_lines(tmp_path):
    path = _plan(tmp_path, "# the four lists\n"
                           "a-reverb a rir=r1\n"
                           "\n"
                           "a-noise a noise=n1:15:0 noise=n2:0:1.5   # two foreground noises\n"
                           "a-music a noise=n2:8:0:bg\n"
                           "a-babble a rir=r2 noise=n1:20:0:bg noise=n2:17:0:bg noise=n1:-3.5:0.25\n"
                           "a-clean a\n")
    entries = augment.read_plan(path, 16000.0, {"r1", "r2"}, {"n1", "n2"})
    assert [(e.out_key, e.src_key, e.rir) for e in entries] == [("a-reverb", "a", "r1"), ("a-noise", "a", None), ("a-music", "a", None),
                                                                ("a-babble", "a", "r2"), ("a-clean", "a", None)]
    assert entries[1].noises == [("n1", 15.0, 0, False), ("n2", 0.0, 24000, False)]
    assert entries[2].noises == [("n2", 8.0, 0, True)]
    assert entries[3].noises == [("n1", 20.0, 0, True), ("n2", 17.0, 0, True), ("n1", -3.5, 4000, False)]
    assert entries[4].noises == []
    # start_seconds * fs is an fp32 product, truncated: 0.3 * 16000 is 4800.0002 in fp32, 0.7 * 16000 is 11199.9996 in double but 11200 in fp32
    assert augment.start_sample(0.3, 16000.0) == 4800 and augment.start_sample(0.7, 16000.0) == int(np.float32(0.7) * np.float32(16000.0))
    # written and read again: the same entries, whatever the start sample
    entries[1].noises.append(("n1", 5.0, 12345, False))
    entries[1].noises.append(("n1", 5.0, 2 ** 21 + 1, False))
    augment.write_plan(entries, str(tmp_path / "again"))
    again = augment.read_plan(str(tmp_path / "again"))
    assert [(e.out_key, e.src_key, e.rir, e.noises) for e in again] == [(e.out_key, e.src_key, e.rir, e.noises) for e in entries]


@pytest.mark.parametrize("line, says", [
    ("only_key", "out_key src_key"),
    ("k a rir=r9", "impulse response r9 is not in the table"),
    ("k a noise=n9:5:0", "noise n9 is not in the table"),
    ("k a rir=r1 rir=r1", "a second impulse response"),
    ("k a noise=n1:5", "noise=ID:snr:start_seconds[:bg]"),
    ("k a noise=n1:5:0:fg", "noise=ID:snr:start_seconds[:bg]"),
    ("k a noise=n1:loud:0", "must be numbers"),
    ("k a noise=n1:5:-1", "start >= 0"),
    ("k a noise=n1:5:2:bg", "its start must be 0"),
    ("k a snr=5", "unknown field `snr=5`"),
    ("k a rir=", "unknown field `rir=`"),
    ("ok a", "output key ok is used twice"),
])
def test_plan_parser_refusals_name_the_line(tmp_path, line, says):
    path = _plan(tmp_path, "ok a rir=r1\n# comment\n" + line + "\n")
    with pytest.raises(ValueError) as e:
        augment.read_plan(path, 16000.0, {"r1"}, {"n1"})
    assert says in str(e.value) and str(e.value).startswith("%s:3: " % path), str(e.value)


def test_make_plan_is_seeded_and_covers_the_four_presets(tmp_path):
    utts = [("u%d" % i, 3.0 + i) for i in range(6)]
    rirs, noises = [("r1", 0.5), ("r2", 1.0)], [("n1", 0.8), ("n2", 2.0), ("n3", 4.0)]
    for preset, snrs in augment.PRESETS.items():
        a = augment.make_plan(preset, utts, rirs, noises, seed=3)
        b = augment.make_plan(preset, utts, rirs, noises, seed=3)
        c = augment.make_plan(preset, utts, rirs, noises, seed=4)
        lines = [e.line(16000.0) for e in a]
        assert lines == [e.line(16000.0) for e in b] and lines != [e.line(16000.0) for e in c]
        assert [e.out_key for e in a] == ["u%d-%s" % (i, preset) for i in range(6)] and [e.src_key for e in a] == [k for k, _ in utts]
        for e, (_, seconds) in zip(a, utts):
            if preset == "reverb":
                assert e.rir in ("r1", "r2") and not e.noises
                continue
            assert e.rir is None and all(n[0] in ("n1", "n2", "n3") and n[1] in snrs for n in e.noises)
            if preset == "noise":
                starts = [n[2] for n in e.noises]
                assert starts[0] == 0 and starts == sorted(starts) and starts[-1] < seconds * 16000 and not any(n[3] for n in e.noises)
                lengths = dict(noises)
                for (nid, _, s0, _), (_, _, s1, _) in zip(e.noises, e.noises[1:]):
                    assert abs(s1 - s0 - (lengths[nid] + 1.0) * 16000) <= 1          # --fg-interval behind the end of the one before
            else:
                assert len(e.noises) == 1 if preset == "music" else 3 <= len(e.noises) <= 7
                assert all(n[2] == 0 and n[3] for n in e.noises)
        augment.write_plan(a, str(tmp_path / preset))
        assert [e.line(16000.0) for e in augment.read_plan(str(tmp_path / preset), 16000.0, dict(rirs), dict(noises))] == lines
    assert {len(e.noises) for e in augment.make_plan("babble", utts * 10, rirs, noises, seed=1)} == {3, 4, 5, 6, 7}
    with pytest.raises(ValueError, match="unknown preset"):
        augment.make_plan("speed", utts, rirs, noises)
    with pytest.raises(ValueError, match="table of impulse responses"):
        augment.make_plan("reverb", utts, [], noises)


def test_options_refusals_are_by_name(tmp_path):
    conf = tmp_path / "augment.conf"
    conf.write_text("--shift-output=false\n--normalize-output=true\n--volume=0.5   # halve\n--impulse-response-channel=1\n--noise-channel=0\n")
    o = augment.AugmentOptions.from_conf(str(conf))
    assert (o.shift_output, o.normalize_output, o.volume, o.impulse_response_channel, o.noise_channel) == (0, 1, 0.5, 1, 0)
    d = augment.AugmentOptions()
    assert (d.shift_output, d.normalize_output, d.volume, d.impulse_response_channel, d.noise_channel) == (1, 1, 0.0, 0, 0)
    cfg = o.config(8000.0)
    assert cfg.struct_bytes == C.sizeof(cfg) == 20 and (cfg.sample_frequency, cfg.shift_output, cfg.normalize_output, cfg.volume) == (8000.0, 0, 1, 0.5)
    for line, says in (("--duration=5", "--duration is not supported: use a background noise entry"),
                       ("--multi-channel-output=true", "--multi-channel-output is not supported"),
                       ("--input-wave-channel=1", "--input-wave-channel is not supported: use --channel of the MFCC conf"),
                       ("--snrs=5:10", "--snrs is not supported"), ("--additive-signals=a.wav", "--additive-signals is not supported"),
                       ("--dither=0", "--dither is not an option of wav-reverberate"), ("--volume=-1", "--volume=-1: must not be negative"),
                       ("--shift-output=maybe", "--shift-output=maybe: true or false is expected")):
        conf.write_text(line + "\n")
        with pytest.raises(ValueError) as e:
            augment.AugmentOptions.from_conf(str(conf))
        assert says in str(e.value), str(e.value)


def test_wav_writer_round_trip(tmp_path):
    rs = np.random.RandomState(5)
    x = rs.randint(-32768, 32768, 4001).astype(np.int16)
    x[:2] = (-32768, 32767)
    path = str(tmp_path / "x.wav")
    augment.write_wav(path, x, 16000.0)
    assert np.array_equal(features.read_wav(path, features.MfccOptions(), "x"), x)
    assert np.array_equal(features.read_wav("cat %s |" % path, features.MfccOptions(channel=0), "x"), x)
    with pytest.raises(ValueError, match="no resampling"):
        features.read_wav(path, features.MfccOptions(sample_frequency=8000.0), "x")
    (tmp_path / "rir.scp").write_text("r1 %s\nr2 cat %s |\n" % (path, path))
    table = augment.read_signals(str(tmp_path / "rir.scp"), 16000.0, 0, "impulse response")
    assert list(table) == ["r1", "r2"] and all(np.array_equal(v, x) for v in table.values())
    with pytest.raises(ValueError, match="no resampling"):
        augment.read_signals(str(tmp_path / "rir.scp"), 8000.0, 0, "impulse response")
    (tmp_path / "twice.scp").write_text("r1 %s\nr1 %s\n" % (path, path))
    with pytest.raises(ValueError, match="listed twice"):
        augment.read_signals(str(tmp_path / "twice.scp"), 16000.0, 0, "noise")


def test_plan_hook_and_workspace_bytes():
    """xv_debug_augment_plan against a restatement of its rule; both entry points are host arithmetic."""
    from tf_kaldi_speaker_amd import _lib, ops
    lib = _lib.load()
    base = ops.augment_plan(1)
    T, KB = base["tile"], base["kb"]
    assert base == dict(tiles=1, tile=T, kb=KB, chain=0) and T % 64 == 0 and KB >= 1
    for n in (1, T - 1, T, T + 1, 2 * T + 3, 320000):
        for L in (0, 1, KB - 1, KB, KB + 1, 3 * KB + 5, 4000, 16000):
            M = n + L - 1 if L else n
            assert ops.augment_plan(n, L) == dict(tiles=-(-M // T), tile=T, kb=KB, chain=KB + -(-L // KB) if L else 0), (n, L)
    for n, L in ((0, 5), (5, -1), (2 ** 31 - 5, 5)):
        with pytest.raises(_lib.XvError, match="augment_plan"):
            ops.augment_plan(n, L)
    # y (a tile's samples in fp32) + a double per tile for E and for Pa, per utterance for P0, per noise entry for Pn
    for b, e, t in ((1, 0, 1), (5, 7, 40), (256, 300, 60000)):
        got = ops.augment_workspace_bytes(b, e, t)
        assert t * T * 4 + 8 * (2 * t + b + e) <= got <= t * T * 4 + 8 * (2 * t + b + e) + 32 and got % 16 == 0
    assert lib.xv_augment_workspace_bytes(-1, 0, 1) == 0
    # the early part: 1 ms in front of the peak, 50 ms behind it, cut at both ends
    h = np.zeros(2000, np.int16)
    h[100] = 9
    h[300] = 9
    assert ops.augment_early(h, 16000.0) == (84, 900, 100) and ops.augment_early(h[:500], 16000.0) == (84, 500, 100)
    assert ops.augment_early(h[90:], 8000.0) == (2, 410, 10) and ops.augment_early(h[100:101], 16000.0) == (0, 1, 0)
