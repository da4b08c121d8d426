"""nnet/lib/extract.py --mfcc-config / --fbank-config on a real MI355X: embeddings straight from a wav.scp against the two-step path it
replaces - make_mfcc.py (make_fbank.py) --compress false to a feature archive and a vad.scp, then extract.py --cmn-window 300 --vad scp: on
them.  Same keys, same order, same log and skip lines, embeddings within the bound tests/test_gpu_extract_batched.py holds batched
against single extraction to (1e-6, its norm); whether they are in fact bit-equal is printed (DESIGN.md section 6c records it).  A tiny
30-dimensional model in both pooling types, as tests/test_gpu_extract_frontend.py builds it.

Six synthetic 16 kHz files: 1.5 s (cut into chunks by --chunk-size 60 after selection), 60 samples (too short for one frame under either
conf: make_mfcc.py drops it, so the wav mode must log that program's skip line), 0.6 s of noise at sigma 2 (log-energy ~7.4 under a
threshold of 5.5 + 0.5 * 7.4: nothing voiced), 0.2 s (20 frames < --min-chunk-size 25), 0.9 s, and 1.2 s behind a `cat file |` pipe."""
import os
import subprocess
import sys
import wave

import numpy as np
import pytest

from tests import mfcc_ref as R
from tests.test_gpu_extract_frontend import _extract, _key_lines, _model, _summary, rel_err

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "tf_kaldi_speaker_amd")
LENS = {"long": 24000, "tiny": 60, "quiet": 9600, "short": 3200, "mid": 14400, "pipe": 19200}
CONF = {"mfcc": "--sample-frequency=16000\n--frame-length=25\n--low-freq=20\n--high-freq=7600\n--num-mel-bins=30\n--num-ceps=30\n--snip-edges=false\n",
        "fbank": "--sample-frequency=16000\n--num-mel-bins=30\n--low-freq=20\n--high-freq=7600\n--dither=0\n"}
COMMON = ["--chunk-size", "60", "--min-chunk-size", "25"]


def _driver(script, args):
    env = dict(os.environ, TF_KALDI_ROOT=PKG, PYTHONPATH=PKG)
    return subprocess.run([sys.executable, os.path.join(PKG, "nnet", "lib", script)] + args, env=env, cwd=PKG, capture_output=True, text=True, timeout=600)


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """The wav.scp, the confs and, per feature kind, the two-step path's first step (run once): feats.ark ('FM '), vad.scp, its log."""
    tmp = tmp_path_factory.mktemp("extract_wav")
    rs = np.random.RandomState(83)
    with open(str(tmp / "wav.scp"), "w") as scp:
        for k, n in LENS.items():
            x = np.rint(rs.randn(n) * 2.0).astype(np.int16) if k == "quiet" else R.signal(rs, n, 16000.0)
            path = str(tmp / (k + ".wav"))
            with wave.open(path, "wb") as w:
                w.setnchannels(1)
                w.setsampwidth(2)
                w.setframerate(16000)
                w.writeframes(x.astype("<i2").tobytes())
            scp.write("%s %s\n" % (k, "cat %s |" % path if k == "pipe" else path))
    (tmp / "vad.conf").write_text("--vad-energy-threshold=5.5\n--vad-energy-mean-scale=0.5\n--vad-proportion-threshold=0.12\n--vad-frames-context=2\n")
    first = {}
    for kind, text in CONF.items():
        (tmp / (kind + ".conf")).write_text(text)
        feats, vad_ark, vad_scp = (str(tmp / (kind + "_" + n)) for n in ("feats.ark", "vad.ark", "vad.scp"))
        r = _driver("make_%s.py" % kind, ["--%s-config" % kind, str(tmp / (kind + ".conf")), "--vad-config", str(tmp / "vad.conf"), "--compress", "false",
                                          str(tmp / "wav.scp"), "ark:" + feats, "ark,scp:%s,%s" % (vad_ark, vad_scp)])
        assert r.returncode == 0, r.stderr[-3000:]
        assert open(feats, "rb").read(10) == b"long \0BFM "
        first[kind] = (feats, vad_scp, r.stderr)
    return tmp, first


@pytest.mark.parametrize("kind", ["mfcc", "fbank"])
@pytest.mark.parametrize("pooling", ["statistics_pooling", "self_attention"], ids=["statistics", "attention"])
def test_wav_mode_equals_the_two_step_path(tmp_path, data, pooling, kind):
    from tf_kaldi_speaker_amd.dataset import kaldi_io
    tmp, first = data
    feats, vad_scp, err_make = first[kind]
    model = str(tmp_path / "exp")
    _model(model, pooling).close()
    out_two, out_wav = str(tmp_path / "two.ark"), str(tmp_path / "wav.ark")
    err_two = _extract(["--cmn-window", "300", "--vad", "scp:" + vad_scp] + COMMON + [model, "ark:" + feats, "ark:" + out_two])
    err_wav = _extract(["--%s-config" % kind, str(tmp / (kind + ".conf")), "--vad-config", str(tmp / "vad.conf"), "--cmn-window", "300"] + COMMON +
                       [model, str(tmp / "wav.scp"), "ark:" + out_wav])
    # the log: the second step's lines, plus the line of the first step for the utterance it dropped, in wav.scp order
    dropped = [ln for ln in _key_lines(err_make) if "too few for one frame" in ln]
    assert dropped == ["Key tiny has 60 samples, too few for one frame, skip."]
    lines_two, lines_wav = _key_lines(err_two), _key_lines(err_wav)
    for ln in lines_wav:
        print(ln)
    assert [ln for ln in lines_wav if ln not in dropped] == lines_two
    assert [ln.split()[1] for ln in lines_wav] == list(LENS)                                  # one line per entry, in wav.scp order
    assert lines_wav[1] == dropped[0] and lines_wav[2] == "Key quiet has no voiced frame, skip."
    assert lines_wav[3].startswith("Key short length too short, ") and lines_wav[3].endswith(" < 25, skip.")
    assert " > 60, split to " in lines_wav[0]
    assert _summary(err_wav) == _summary(err_two)                                              # utterances and (post-selection) frames
    two, wav = list(kaldi_io.read_vec_flt_ark(out_two)), list(kaldi_io.read_vec_flt_ark(out_wav))
    assert [k for k, _ in wav] == [k for k, _ in two] == ["long", "mid", "pipe"]
    worst = 0.0
    for (k, a), (_, b) in zip(wav, two):
        assert np.abs(b).max() > 1e-3
        worst = max(worst, rel_err(a, b.astype(np.float64)))
    print("%s %s: worst relative difference wav mode against the two-step path %.3g; output files bit-equal: %s"
          % (kind, pooling, worst, open(out_wav, "rb").read() == open(out_two, "rb").read()))
    assert worst <= 1e-6, worst
    if kind == "fbank":
        return
    # without --vad-config every frame is kept: the two-step path without --vad
    out_two_all, out_wav_all = str(tmp_path / "two_all.ark"), str(tmp_path / "wav_all.ark")
    err_two_all = _extract(["--cmn-window", "300"] + COMMON + [model, "ark:" + feats, "ark:" + out_two_all])
    err_wav_all = _extract(["--mfcc-config", str(tmp / "mfcc.conf"), "--cmn-window", "300"] + COMMON + [model, str(tmp / "wav.scp"), "ark:" + out_wav_all])
    assert [ln for ln in _key_lines(err_wav_all) if ln not in dropped] == _key_lines(err_two_all)
    two, wav = list(kaldi_io.read_vec_flt_ark(out_two_all)), list(kaldi_io.read_vec_flt_ark(out_wav_all))
    assert [k for k, _ in wav] == [k for k, _ in two] == ["long", "quiet", "mid", "pipe"]
    for (k, a), (_, b) in zip(wav, two):
        assert rel_err(a, b.astype(np.float64)) <= 1e-6, (k, rel_err(a, b.astype(np.float64)))


def test_wav_mode_refusals(tmp_path, data):
    tmp, first = data
    _model(str(tmp_path / "real")).close()
    mfcc, fbank, vad, scp = (str(tmp / n) for n in ("mfcc.conf", "fbank.conf", "vad.conf", "wav.scp"))
    out = "ark:" + str(tmp_path / "never.ark")
    (tmp_path / "mfcc13.conf").write_text(CONF["mfcc"].replace("--num-ceps=30", "--num-ceps=13"))
    (tmp_path / "dither.conf").write_text(CONF["fbank"].replace("--dither=0", "--dither=1"))
    (tmp_path / "bad.scp").write_text("only_a_key\n")
    (tmp_path / "rate.scp").write_text("k %s\n" % str(tmp / "long.wav"))
    (tmp_path / "mfcc8k.conf").write_text(CONF["mfcc"].replace("16000", "8000").replace("7600", "3700"))
    real = str(tmp_path / "real")
    for args, words in (
            (["--mfcc-config", mfcc, "--vad-config", vad, "--vad", "scp:" + first["mfcc"][1], real, scp, out], ("--vad", "--vad-config")),
            (["--mfcc-config", mfcc, "--vad", "scp:" + first["mfcc"][1], real, scp, out], ("--vad ", "--vad-config")),
            (["--mfcc-config", mfcc, "--fbank-config", fbank, real, scp, out], ("--mfcc-config and --fbank-config", "exactly one")),
            (["--vad-config", vad, real, "ark:" + first["mfcc"][0], out], ("--vad-config", "--mfcc-config or --fbank-config")),
            (["--mfcc-config", mfcc, real, "ark:" + first["mfcc"][0], out], ("wav.scp", "ark:")),
            (["--fbank-config", fbank, real, "ark:" + first["fbank"][0], out], ("wav.scp", "ark:")),
            (["--mfcc-config", str(tmp_path / "mfcc13.conf"), real, scp, out], ("--mfcc-config", "13 dimensions", "nnet/feature_dim is 30")),
            (["--fbank-config", str(tmp_path / "dither.conf"), real, scp, out], ("--dither=1", "not supported")),
            (["--mfcc-config", mfcc, real, str(tmp_path / "bad.scp"), out], ("`key rxfilename` is expected", "only_a_key")),
            (["--mfcc-config", str(tmp_path / "mfcc8k.conf"), real, str(tmp_path / "rate.scp"), out], ("Key k", "16000 Hz", "--allow-downsample=true"))):
        r = _driver("extract.py", args)
        assert r.returncode != 0, args
        refusal = [ln for ln in r.stderr.splitlines() if "INFO:" not in ln]      # what sys.exit wrote, beside the log lines
        for word in words:
            assert any(word in ln for ln in refusal), (args, word, r.stderr[-1000:])
        assert "Traceback" not in r.stderr, r.stderr[-2000:]
    assert not os.path.exists(str(tmp_path / "never.ark")) or os.path.getsize(str(tmp_path / "never.ark")) == 0


def test_make_fbank_without_the_vad_table(tmp_path, data):
    """make_fbank.py with the VAD wspecifier left out and --compress true: no decisions are computed or logged, the frame counts come from
    the features, and the 'CM ' archive holds the 'FM ' features of the run with the table within the codec's step, (max - min) / 255 of a column."""
    from tf_kaldi_speaker_amd.dataset import kaldi_io
    tmp, first = data
    feats, counts = str(tmp_path / "fbank_cm.ark"), str(tmp_path / "utt2num_frames")
    r = _driver("make_fbank.py", ["--fbank-config", str(tmp / "fbank.conf"), "--compress", "true", "--write-utt2num-frames", counts, str(tmp / "wav.scp"),
                                  "ark:" + feats])
    assert r.returncode == 0, r.stderr[-3000:]
    lines = _key_lines(r.stderr)
    assert [ln.split()[1].rstrip(":") for ln in lines] == list(LENS) and not any("voiced" in ln for ln in lines)
    assert "Key tiny has 60 samples, too few for one frame, skip." in lines and "voiced" not in r.stderr.split("Computed features of")[1]
    want = dict(kaldi_io.read_mat_ark(first["fbank"][0]))
    got = list(kaldi_io.read_mat_ark(feats))
    assert open(feats, "rb").read(10) == b"long \0BCM " and [k for k, _ in got] == [k for k in LENS if k != "tiny"] == list(want)
    assert [ln.split() for ln in open(counts)] == [[k, str(len(want[k]))] for k in want]
    for k, m in got:
        assert m.shape == want[k].shape == (1 + (LENS[k] - 400) // 160, 30)
        step = (want[k].max(axis=0) - want[k].min(axis=0)) / 255.0
        assert (np.abs(m - want[k]) <= step + 1e-6 * np.abs(want[k])).all(), k
        assert "Key %s: %d samples, %d frames." % (k, LENS[k], len(m)) in lines


def test_wav_mode_with_a_resampled_file_equals_the_two_step_path(tmp_path, data):
    """An 8 kHz file among the 16 kHz ones under --allow-upsample=true: it is resampled on the device and its features sit in a second
    feature call, so one extraction window draws on two device batches - still planned, padded and run as the two-step path runs them."""
    from tf_kaldi_speaker_amd.dataset import kaldi_io
    tmp, _ = data
    low = str(tmp_path / "low.wav")
    with wave.open(low, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(8000)
        w.writeframes(R.signal(np.random.RandomState(89), 8000, 8000.0).astype("<i2").tobytes())
    lines = open(str(tmp / "wav.scp")).read().splitlines()
    scp = str(tmp_path / "wav.scp")
    open(scp, "w").write("\n".join(lines[:3] + ["low " + low] + lines[3:]) + "\n")
    conf = str(tmp_path / "mfcc.conf")
    open(conf, "w").write(CONF["mfcc"] + "--allow-upsample=true\n")
    feats, vad_scp = str(tmp_path / "feats.ark"), str(tmp_path / "vad.scp")
    r = _driver("make_mfcc.py", ["--mfcc-config", conf, "--vad-config", str(tmp / "vad.conf"), "--compress", "false", scp, "ark:" + feats,
                                 "ark,scp:%s,%s" % (str(tmp_path / "vad.ark"), vad_scp)])
    assert r.returncode == 0, r.stderr[-3000:]
    note = "Key low: resampled from 8000 Hz."
    assert note in _key_lines(r.stderr)
    model = str(tmp_path / "exp")
    _model(model).close()
    out_two, out_wav = str(tmp_path / "two.ark"), str(tmp_path / "wav.ark")
    err_two = _extract(["--cmn-window", "300", "--vad", "scp:" + vad_scp] + COMMON + [model, "ark:" + feats, "ark:" + out_two])
    err_wav = _extract(["--mfcc-config", conf, "--vad-config", str(tmp / "vad.conf"), "--cmn-window", "300"] + COMMON + [model, scp, "ark:" + out_wav])
    lines_wav = _key_lines(err_wav)
    assert note in lines_wav
    assert [ln for ln in lines_wav if ln != note and "too few for one frame" not in ln] == _key_lines(err_two)
    assert _summary(err_wav) == _summary(err_two)
    two, wav = list(kaldi_io.read_vec_flt_ark(out_two)), list(kaldi_io.read_vec_flt_ark(out_wav))
    assert [k for k, _ in wav] == [k for k, _ in two] == ["long", "low", "mid", "pipe"]
    worst = max(rel_err(a, b.astype(np.float64)) for (_, a), (_, b) in zip(wav, two))
    print("two device batches in one window: worst relative difference %.3g; output files bit-equal: %s"
          % (worst, open(out_wav, "rb").read() == open(out_two, "rb").read()))
    assert worst <= 1e-6, worst
