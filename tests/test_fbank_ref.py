"""CPU checks of the filterbank stage: the restatement tests/fbank_ref.py tied to the pinned tests/mfcc_ref.py (its log-mel columns times
that module's DCT and lifter are that module's MFCCs), the host arithmetic of the library - xv_fbank_tables, xv_fbank_num_frames: the
library loads without a GPU - against the restatement, the conf parser of misc/features.py, the refusal of more than 128 columns, and the
command lines of the two drivers that take the new options."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import fbank_ref as FB
from tests import mfcc_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "tf_kaldi_speaker_amd")

CONFIGS = {"defaults": FB.config(), "voxceleb30": FB.config(num_mel_bins=30, high_freq=7600.0, snip_edges=0),
           "sre_energy": FB.config(sample_frequency=8000.0, high_freq=3700.0, use_energy=1, raw_energy=0, energy_floor=2.0),
           "n128": FB.config(frame_length_ms=5.0, frame_shift_ms=2.0, num_mel_bins=40, high_freq=7600.0),
           "d128": FB.config(num_mel_bins=127, use_energy=1, snip_edges=0)}


@pytest.mark.parametrize("name", ["defaults", "voxceleb30", "sre_energy"])
def test_log_mel_times_dct_is_the_pinned_mfcc(name):
    """fbank (log, power) @ (DCT . lifter)^T == mfcc_ref.mfcc to 1e-12 relative; with use_energy both carry the same column 0, and the
    energy handed to energy_out is that column whatever use_energy says."""
    cfg = dict(CONFIGS[name])
    x = R.signal(np.random.RandomState(5), 4000, cfg["sample_frequency"])
    for use_energy in (0, 1):
        cfg["use_energy"] = use_energy
        mcfg = FB.as_mfcc(cfg, cepstral_lifter=22.0, num_ceps=min(cfg["num_mel_bins"], 20))
        want = R.mfcc(x, mcfg)
        got, log_e = FB.fbank(x, cfg, with_energy=True)
        assert got.shape == (R.num_frames(4000, mcfg), cfg["num_mel_bins"] + use_energy) and len(got) > 5
        c = got[:, use_energy:] @ R.tables(mcfg)["dct"].T
        if use_energy:
            assert np.array_equal(got[:, 0], want[:, 0]) and np.array_equal(got[:, 0], log_e)
            c[:, 0] = got[:, 0]
        else:
            assert np.array_equal(log_e, R.mfcc(x, dict(mcfg, use_energy=1))[:, 0])
        assert np.abs(c - want).max() <= 1e-12 * np.abs(want).max()


def test_restatement_options():
    """use_log_fbank off gives the energies themselves, use_power off sums magnitudes; fp32 runs in fp32 and stays near fp64."""
    x = R.signal(np.random.RandomState(6), 3000, 16000.0)
    log_pow, lin_pow = FB.fbank(x, FB.config()), FB.fbank(x, FB.config(use_log_fbank=0))
    assert np.allclose(np.log(np.maximum(lin_pow, FB.EPS)), log_pow, rtol=0, atol=1e-12) and lin_pow.min() > 1.0
    lin_mag = FB.fbank(x, FB.config(use_log_fbank=0, use_power=0))
    assert (lin_mag < lin_pow).all() and (lin_mag ** 2 <= lin_pow * 40).all()      # a sum of <= ~40 magnitudes against the sum of their squares
    a, b = FB.fbank(x, FB.config(use_energy=1)), FB.fbank(x, FB.config(use_energy=1), np.float32)
    assert a.dtype == np.float64 and b.dtype == np.float32 and a.shape == b.shape == (17, 24)
    assert 1e-8 < np.abs(a - b).max() < 1e-2
    quiet = FB.fbank(np.zeros(800, np.int16), FB.config(use_energy=1, energy_floor=1.0))
    assert np.array_equal(quiet[:, 0], np.zeros(3)) and np.allclose(quiet[:, 1:], np.log(FB.EPS))


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_library_tables_equal_the_restatement_bit_for_bit(name):
    """xv_fbank_tables == the restated tables (fp64, packed in the library's layout) after ONE rounding to fp32, bit for bit - and ==
    xv_mfcc_tables' leading blocks for the shared fields, bit for bit (the kernel body is one: its tables must be too)."""
    from tf_kaldi_speaker_amd import _lib
    cfg = CONFIGS[name]
    lib = _lib.load()
    c = _lib.XvFbankConfig(**cfg)
    n = lib.xv_fbank_table_floats(C.byref(c))
    assert n > 0, lib.xv_last_error()
    flat = np.full(n, np.nan, np.float32)
    assert lib.xv_fbank_tables(C.byref(c), flat.ctypes.data_as(C.c_void_p), n) == 0, lib.xv_last_error()
    assert np.isfinite(flat).all()
    ref = FB.pack_tables(FB.tables(cfg))
    assert ref.shape == flat.shape
    L, S, N = FB.dims(cfg)
    bins = cfg["num_mel_bins"]
    idx = slice(L + N, L + N + 3 * bins)
    assert np.array_equal(flat[idx], ref[idx].astype(np.float32))                       # first / count / offset: whole numbers, exact
    ref32 = ref.astype(np.float32)                                                         # the one rounding
    differ = np.flatnonzero(flat.view(np.uint32) != ref32.view(np.uint32))
    print("%s: %d of %d table entries differ from the restatement" % (name, len(differ), n))
    assert len(differ) == 0, (differ[:8], flat[differ[:8]], ref32[differ[:8]])
    assert (FB.tables(cfg)["mel_count"].min() == 0) == (name in ("n128", "d128"))      # both carry mel bins that hold no FFT bin
    # the same numbers as xv_mfcc_tables for the same fields
    m = _lib.XvMfccConfig(**FB.as_mfcc(cfg, num_ceps=1))
    nm = lib.xv_mfcc_table_floats(C.byref(m))
    assert nm == n + bins
    mflat = np.empty(nm, np.float32)
    assert lib.xv_mfcc_tables(C.byref(m), mflat.ctypes.data_as(C.c_void_p), nm) == 0
    assert np.array_equal(mflat[:n].view(np.uint32), flat.view(np.uint32))
    assert lib.xv_fbank_tables(C.byref(c), flat.ctypes.data_as(C.c_void_p), n - 1) != 0 and b"floats" in lib.xv_last_error()
    got = FB.unpack_tables(flat, cfg)
    assert np.array_equal(got["mel_first"], FB.tables(cfg)["mel_first"]) and np.array_equal(got["mel_count"], FB.tables(cfg)["mel_count"])


@pytest.mark.parametrize("snip_edges", [1, 0])
def test_library_frame_counts(snip_edges):
    from tf_kaldi_speaker_amd import _lib
    lib = _lib.load()
    for base in (FB.config(), FB.config(sample_frequency=8000.0, high_freq=3700.0), FB.config(frame_length_ms=64.0, frame_shift_ms=16.0)):
        cfg = dict(base, snip_edges=snip_edges)
        L, S, _ = FB.dims(cfg)
        c = _lib.XvFbankConfig(**cfg)
        for n in (0, L - 1, L, L + 1, L + S):
            assert lib.xv_fbank_num_frames(C.byref(c), n) == R.num_frames(n, cfg), (cfg, n)
    assert [R.num_frames(n, FB.config()) for n in (399, 400, 401, 560)] == [0, 1, 1, 2]


def test_library_refuses_by_name():
    from tf_kaldi_speaker_amd import _lib
    lib = _lib.load()
    for kw, word in ((dict(num_mel_bins=128, use_energy=1), "129 columns"), (dict(num_mel_bins=129), "num_mel_bins"), (dict(frame_length_ms=100.0), "frame_length_ms"),
                     (dict(high_freq=9000.0), "high_freq"), (dict(low_freq=-1.0), "low_freq"), (dict(energy_floor=-1.0), "energy_floor")):
        c = _lib.XvFbankConfig(**kw)
        assert lib.xv_fbank_table_floats(C.byref(c)) == 0 and word in lib.xv_last_error().decode(), kw
        assert lib.xv_last_error().decode().startswith("fbank:")
        assert lib.xv_fbank_num_frames(C.byref(c), 16000) == -1
    assert lib.xv_fbank_table_floats(C.byref(_lib.XvFbankConfig(num_mel_bins=128))) > 0              # d = 128 without the energy column
    assert lib.xv_fbank_table_floats(C.byref(_lib.XvFbankConfig(num_mel_bins=127, use_energy=1))) > 0
    c = _lib.XvFbankConfig()
    c.struct_bytes -= 4
    assert lib.xv_fbank_table_floats(C.byref(c)) == 0 and "struct_bytes" in lib.xv_last_error().decode()
    # the MFCC entry points keep their messages
    m = _lib.XvMfccConfig(num_ceps=0)
    assert lib.xv_mfcc_table_floats(C.byref(m)) == 0 and lib.xv_last_error().decode().startswith("mfcc: num_ceps")


def test_ops_fbank_refuses_more_than_128_columns():
    from tf_kaldi_speaker_amd import _lib, ops
    with pytest.raises(_lib.XvError, match="129 columns"):
        ops.fbank_tables(ops.fbank_config(num_mel_bins=128, use_energy=1))
    with pytest.raises(_lib.XvError, match="129 columns"):
        ops.fbank_num_frames(ops.fbank_config(num_mel_bins=128, use_energy=1), 16000)
    assert ops.fbank_tables(ops.fbank_config()).dtype == np.float32 and ops.fbank_num_frames(ops.fbank_config(), 560) == 2


def test_fbank_options_parse_a_conf_and_refuse_by_name(tmp_path):
    from tf_kaldi_speaker_amd.misc import features
    o = features.FbankOptions()
    assert {k: getattr(o, k) for k in FB.DEFAULTS} == FB.DEFAULTS and o.feature_dim() == 23 and o.KIND == "fbank"
    conf = tmp_path / "fbank.conf"
    conf.write_text("--sample-frequency=16000\n--num-mel-bins=40 # no default here\n--low-freq=20\n--high-freq=-400\n--snip-edges=false\n"
                    "--use-energy=true\n--use-log-fbank=true\n--use-power=false\n--energy-floor=1.5\n\n--dither=0\n--allow-downsample=true\n")
    o = features.FbankOptions.from_conf(str(conf))
    assert (o.num_mel_bins, o.high_freq, o.snip_edges, o.use_energy, o.use_log_fbank, o.use_power, o.energy_floor, o.allow_downsample) == \
        (40, -400.0, 0, 1, 1, 0, 1.5, 1)
    assert o.feature_dim() == 41
    cfg = o.config()
    assert cfg.num_mel_bins == 40 and cfg.use_power == 0 and cfg.struct_bytes == C.sizeof(type(cfg)) and not hasattr(cfg, "channel")
    for line, word in (("--dither=1.0", "dither"), ("--window-type=hamming", "window-type"), ("--htk-compat=true", "htk-compat"),
                       ("--round-to-power-of-two=false", "round-to-power-of-two"), ("--vtln-warp=1.1", "vtln-warp"), ("--vtln-low=60", "vtln-low"),
                       ("--subtract-mean=true", "subtract-mean"), ("--num-ceps=13", "num-ceps"), ("--cepstral-lifter=22", "cepstral-lifter"),
                       ("--no-such-option=3", "no-such-option")):
        bad = tmp_path / "bad.conf"
        bad.write_text("--num-mel-bins=40\n" + line + "\n")
        with pytest.raises(ValueError, match="--" + word):
            features.FbankOptions.from_conf(str(bad))
    with pytest.raises(ValueError, match="compute-fbank-feats"):
        features.FbankOptions().set("num-ceps", "13")
    assert features.MfccOptions().feature_dim() == 30 and features.MfccOptions.KIND == "mfcc"


def _help(script):
    env = dict(os.environ, TF_KALDI_ROOT=PKG, PYTHONPATH=PKG)
    r = subprocess.run([sys.executable, os.path.join(PKG, "nnet", "lib", script), "--help"], env=env, cwd=PKG, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout


def test_make_fbank_help():
    out = _help("make_fbank.py")
    for word in ("--fbank-config", "--vad-config", "--compress", "--write-utt2num-frames", "--augment-plan", "wav_scp", "feats_wspecifier", "[vad_wspecifier]"):
        assert word in out, word
    assert "--mfcc-config" not in out


def test_extract_help_names_the_wav_options():
    out = _help("extract.py")
    for word in ("--mfcc-config", "--fbank-config", "--vad-config", "--cmn-window", "--vad "):
        assert word in out, word
