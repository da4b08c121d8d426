"""CPU checks of the MFCC / VAD stage: the fp64 restatement (tests/mfcc_ref.py) held against its own literal per-sample loops, the frame
counts, the constant tables of xv_mfcc_tables (host arithmetic: the library loads without a GPU) against the restatement's, the Kaldi conf
parser and the wav reader of misc/features.py, the driver's command line, and the VAD restatement against a hand-worked mask."""
import ctypes as C
import os
import subprocess
import sys
import wave

import numpy as np
import pytest

from tests import mfcc_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "tf_kaldi_speaker_amd")


@pytest.mark.parametrize("snip_edges", [1, 0])
@pytest.mark.parametrize("n", [80, 81, 399, 400, 401, 560])
def test_vectorised_restatement_equals_the_loops(n, snip_edges):
    cfg = R.config(snip_edges=snip_edges)
    x = R.signal(np.random.RandomState(n), n, 16000.0)
    a, b = R.gather(x, cfg), R.gather_loop(x, cfg)
    assert a.shape == b.shape == (R.num_frames(n, cfg), 400)
    assert np.array_equal(a, b)
    if len(a):
        for dt in (np.float64, np.float32):
            assert np.array_equal(R.preemphasize(a.astype(dt), 0.97), R.preemphasize_loop(a.astype(dt), 0.97))
    else:
        assert snip_edges and n < 400


def test_frame_counts():
    on, off = R.config(snip_edges=1), R.config(snip_edges=0)
    assert [R.num_frames(n, on) for n in (399, 400, 560)] == [0, 1, 2]
    assert [R.num_frames(n, off) for n in (79, 80, 240, 400)] == [0, 1, 2, 3]
    assert R.dims(R.VOXCELEB) == (400, 160, 512) and R.dims(R.SRE) == (200, 80, 256)
    from tf_kaldi_speaker_amd import _lib
    lib = _lib.load()
    for cfg in (on, off, R.SRE, R.THIRD):
        c = _lib.XvMfccConfig(**cfg)
        for n in (0, 1, 79, 80, 81, 199, 200, 239, 240, 399, 400, 401, 560, 16000, 48037):
            assert lib.xv_mfcc_num_frames(C.byref(c), n) == R.num_frames(n, cfg), (cfg, n)


def _ulps(got, ref64):
    ref = np.asarray(ref64, np.float64).astype(np.float32)
    return float((np.abs(np.asarray(got, np.float64) - ref.astype(np.float64)) / np.spacing(np.abs(ref)).astype(np.float64)).max())


@pytest.mark.parametrize("name", sorted(R.CONFIGS))
def test_library_tables_equal_the_restatement(name):
    from tf_kaldi_speaker_amd import _lib
    cfg = R.CONFIGS[name]
    lib = _lib.load()
    c = _lib.XvMfccConfig(**cfg)
    n = lib.xv_mfcc_table_floats(C.byref(c))
    assert n > 0, lib.xv_last_error()
    flat = np.full(n, np.nan, np.float32)
    assert lib.xv_mfcc_tables(C.byref(c), flat.ctypes.data_as(C.c_void_p), n) == 0, lib.xv_last_error()
    assert np.isfinite(flat).all()
    got, ref = R.unpack_tables(flat, cfg), R.tables(cfg)
    assert np.array_equal(got["mel_first"], ref["mel_first"]) and np.array_equal(got["mel_count"], ref["mel_count"])
    assert ref["mel_count"].min() > 0
    assert _ulps(got["window"], ref["window"]) <= 1
    assert _ulps(got["dct"], ref["dct"]) <= 1
    for m in range(cfg["num_mel_bins"]):
        assert _ulps(got["mel_weights"][m], ref["mel_weights"][m]) <= 1, m
    # the twiddles pass through zero: one ulp of 1.0 in absolute terms
    assert np.abs(got["twiddles"].astype(np.float64) - ref["twiddles"]).max() <= 2.0 ** -23
    # each FFT bin lies in at most two triangles
    assert (np.count_nonzero(ref["mel_dense"], axis=0) <= 2).all()
    assert lib.xv_mfcc_tables(C.byref(c), flat.ctypes.data_as(C.c_void_p), n - 1) != 0 and b"floats" in lib.xv_last_error()


def test_library_refuses_what_it_does_not_support_by_name():
    from tf_kaldi_speaker_amd import _lib
    lib = _lib.load()
    for kw, word in ((dict(frame_length_ms=100.0), "frame_length_ms"), (dict(frame_length_ms=2.0), "frame_length_ms"), (dict(num_mel_bins=129), "num_mel_bins"),
                     (dict(num_ceps=31), "num_ceps"), (dict(high_freq=9000.0), "high_freq"), (dict(low_freq=-1.0), "low_freq")):
        c = _lib.XvMfccConfig(**kw)
        assert lib.xv_mfcc_table_floats(C.byref(c)) == 0 and word in lib.xv_last_error().decode(), kw
        assert lib.xv_mfcc_num_frames(C.byref(c), 16000) == -1
    c = _lib.XvMfccConfig()
    c.struct_bytes -= 4
    assert lib.xv_mfcc_table_floats(C.byref(c)) == 0 and "struct_bytes" in lib.xv_last_error().decode()


def test_mfcc_options_parse_a_conf_and_refuse_by_name(tmp_path):
    from tf_kaldi_speaker_amd.misc import features
    conf = tmp_path / "mfcc.conf"
    conf.write_text("--sample-frequency=16000\n--frame-length=25 # the default is 25\n--low-freq=20 # the default.\n"
                    "--high-freq=7600 # the default is zero meaning use the Nyquist (8k in this case).\n--num-mel-bins=30\n--num-ceps=30\n"
                    "--snip-edges=false\n\n--dither=0\n")
    o = features.MfccOptions.from_conf(str(conf))
    assert {k: getattr(o, k) for k in R.DEFAULTS} == R.VOXCELEB
    cfg = o.config()
    assert cfg.num_ceps == 30 and cfg.snip_edges == 0 and cfg.high_freq == 7600.0 and cfg.struct_bytes == C.sizeof(type(cfg))
    sre = tmp_path / "sre.conf"
    sre.write_text("--sample-frequency=8000\n--frame-length=25\n--low-freq=20\n--high-freq=3700\n--num-ceps=23\n--num-mel-bins=23\n--snip-edges=true\n")
    o = features.MfccOptions.from_conf(str(sre))
    assert (o.sample_frequency, o.num_ceps, o.num_mel_bins, o.high_freq, o.snip_edges) == (8000.0, 23, 23, 3700.0, 1)
    for line, word in (("--dither=1.0", "dither"), ("--window-type=hamming", "window-type"), ("--htk-compat=true", "htk-compat"),
                       ("--round-to-power-of-two=false", "round-to-power-of-two"), ("--vtln-warp=1.1", "vtln-warp"), ("--subtract-mean=true", "subtract-mean"),
                       ("--no-such-option=3", "no-such-option")):
        bad = tmp_path / "bad.conf"
        bad.write_text("--num-ceps=30\n" + line + "\n")
        with pytest.raises(ValueError, match="--" + word):
            features.MfccOptions.from_conf(str(bad))
    vad = tmp_path / "vad.conf"
    vad.write_text("--vad-energy-threshold=5.5\n--vad-energy-mean-scale=0.5\n--vad-proportion-threshold=0.12\n--vad-frames-context=2\n")
    v = features.VadOptions.from_conf(str(vad))
    assert (v.threshold, v.mean_scale, v.proportion, v.frames_context) == (5.5, 0.5, 0.12, 2)
    vad.write_text("--vad-energy-threshold=5.5\n--dither=0\n")
    with pytest.raises(ValueError, match="--dither"):
        features.VadOptions.from_conf(str(vad))


def _write_wav(path, x, rate=16000, width=2):
    x = np.asarray(x)
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1 if x.ndim == 1 else x.shape[1])
        w.setsampwidth(width)
        w.setframerate(rate)
        w.writeframes(x.astype("<i2" if width == 2 else np.uint8).tobytes())


def test_read_wav_round_trip_and_refusals(tmp_path):
    from tf_kaldi_speaker_amd.misc import features
    x = R.signal(np.random.RandomState(3), 1234, 16000.0)
    _write_wav(tmp_path / "a.wav", x)
    got = features.read_wav(str(tmp_path / "a.wav"))
    assert got.dtype == np.int16 and np.array_equal(got, x)
    assert np.array_equal(features.read_wav("cat %s |" % (tmp_path / "a.wav"), key="piped"), x)
    stereo = np.stack([x, -x], axis=1)
    _write_wav(tmp_path / "s.wav", stereo)
    with pytest.raises(ValueError, match="Key st .*2 channels"):
        features.read_wav(str(tmp_path / "s.wav"), key="st")
    assert np.array_equal(features.read_wav(str(tmp_path / "s.wav"), features.MfccOptions(channel=1)), -x)
    _write_wav(tmp_path / "b.wav", (x >> 8) + 128, width=1)
    with pytest.raises(ValueError, match="Key eight .*8-bit"):
        features.read_wav(str(tmp_path / "b.wav"), key="eight")
    _write_wav(tmp_path / "r.wav", x, rate=8000)
    with pytest.raises(ValueError, match="Key slow .*8000 Hz"):
        features.read_wav(str(tmp_path / "r.wav"), key="slow")
    (tmp_path / "junk.wav").write_bytes(b"not a wave file at all")
    with pytest.raises(ValueError, match="Key junk .*RIFF"):
        features.read_wav(str(tmp_path / "junk.wav"), key="junk")


def test_make_mfcc_help():
    env = dict(os.environ, TF_KALDI_ROOT=PKG, PYTHONPATH=PKG)
    r = subprocess.run([sys.executable, os.path.join(PKG, "nnet", "lib", "make_mfcc.py"), "--help"], env=env, cwd=PKG, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    for word in ("--mfcc-config", "--vad-config", "--compress", "--write-utt2num-frames", "wav_scp", "feats_wspecifier", "vad_wspecifier"):
        assert word in r.stdout, word


def test_vad_restatement_on_a_hand_worked_vector():
    e = np.array([10.0, 10.0, 0.0, 0.0, 0.0, 0.0, 0.0, 10.0, 0.0, 0.0])
    feats = np.stack([e, np.full(10, 99.0)], axis=1)
    # mean 3, threshold 2 + 0.5 * 3 = 3.5: frames 0, 1 and 7 lie above.  Context 1, proportion 0.5: a window needs at least half of its frames above.
    #   t:      0    1    2    3    4    5    6    7    8    9
    #   above:  2/2  2/3  1/3  0/3  0/3  0/3  1/3  1/3  1/3  0/2
    assert R.vad_threshold(e, 2.0, 0.5) == 3.5
    assert R.energy_vad(feats, 2.0, 0.5, 1, 0.5).tolist() == [1, 1, 0, 0, 0, 0, 0, 0, 0, 0]
    # proportion 0.3: one of three is enough, one of two as well
    assert R.energy_vad(feats, 2.0, 0.5, 1, 0.3).tolist() == [1, 1, 1, 0, 0, 0, 1, 1, 1, 0]
    # no mean, no context, proportion 1: the comparison alone (strictly above)
    assert R.energy_vad(feats, 10.0, 0.0, 0, 1.0).tolist() == [0] * 10
    assert R.energy_vad(feats, 9.5, 0.0, 0, 1.0).tolist() == [1, 1, 0, 0, 0, 0, 0, 1, 0, 0]
    # context 2 at both ends of a 4-frame vector: the windows are cut to the vector
    assert R.energy_vad(np.array([[9.0], [0.0], [0.0], [0.0]]), 5.0, 0.0, 2, 0.3).tolist() == [1, 0, 0, 0]
    assert R.energy_vad(np.array([[9.0], [0.0], [0.0], [0.0]]), 5.0, 0.0, 2, 0.25).tolist() == [1, 1, 1, 0]


def test_restatement_in_fp32_stays_near_fp64_and_the_floors_hold():
    """The dtype switch really runs in single precision, and digital silence sits at the FLT_EPSILON floors (--energy-floor lifts column 0)."""
    x = R.signal(np.random.RandomState(1), 4000, 16000.0)
    a, b = R.mfcc(x, R.VOXCELEB), R.mfcc(x, R.VOXCELEB, np.float32)
    assert a.dtype == np.float64 and b.dtype == np.float32 and a.shape == b.shape == (25, 30)
    d = np.abs(a - b).max()
    assert 1e-7 < d < 1e-2, d
    quiet = R.mfcc(np.zeros(800, np.int16), R.VOXCELEB)
    assert np.allclose(quiet[:, 0], np.log(R.EPS)) and np.abs(quiet[:, 1:]).max() < 1e-9
    floored = R.mfcc(np.zeros(800, np.int16), R.config(energy_floor=1.0))
    assert np.array_equal(floored[:, 0], np.zeros(5))


def test_compressed_writer_uniform_header_bounds_the_error_and_the_default_is_unchanged():
    """write_compressed_mat(header="uniform"), what make_mfcc.py --compress true writes.  With g = (matrix range) / 65535 the header's grid, the
    end points rounded outwards span at most range + 2 g, a quarter of that (rounded: + g / 2) carries 63 codes at the coarsest, so the error
    is at most (range / 4 + g) / 126 <= range / 255 for every column with range >= 5 g - whatever its distribution; the quartile header
    (the default, Kaldi's ComputeColHeader) misses that on skewed columns.  The default's bytes are what they were."""
    import io
    from tf_kaldi_speaker_amd.dataset import kaldi_io
    rs = np.random.RandomState(61)
    rows = 400
    m = np.stack([rs.randn(rows) * 30, rs.exponential(1.0, rows) ** 3, np.where(rs.rand(rows) < 0.2, 14.0, 21.6) + rs.randn(rows) * 0.01,
                  rs.rand(rows) * 0.05 + 20.0, np.r_[np.zeros(rows - 1), 150.0], rs.randn(rows)], axis=1).astype(np.float32)
    g = float(m.max() - m.min()) / 65535.0
    rng = (m.max(axis=0) - m.min(axis=0)).astype(np.float64)
    assert rng.min() >= 5 * g and rng.min() < 16 * g                    # one column close to the grid
    out = {}
    for header in ("quartiles", "uniform", None):
        buf = io.BytesIO()
        kaldi_io.write_compressed_mat(buf, m, key="k", **({} if header is None else {"header": header}))
        out[header] = buf.getvalue()
        buf.seek(0)
        back = dict(kaldi_io.read_mat_ark(buf))["k"]
        ratio = np.abs(back.astype(np.float64) - m).max(axis=0) / (rng / 255.0)
        if header == "uniform":
            assert ratio.max() <= 1.0, ratio
        elif header == "quartiles":
            assert ratio.max() > 1.5, ratio                               # the skewed columns
    assert out[None] == out["quartiles"] != out["uniform"]
    with pytest.raises(ValueError, match="header"):
        kaldi_io.write_compressed_mat(io.BytesIO(), m, header="even")
