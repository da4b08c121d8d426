"""nnet/lib/make_mfcc.py on a real MI355X: a six-utterance wav.scp (one entry a `cat file |` pipe) to the feature and VAD tables with
--compress=true, read back with kaldi_io and held against the fp64 restatement (tests/mfcc_ref.py): keys, order, frame counts,
utt2num_frames, VAD decisions equal; the features against the restatement; then extract.py --cmn-window 300 --vad scp: must accept the two
files and write one vector per key.  The driver runs once for the module."""
import io
import os
import subprocess
import sys
import wave

import numpy as np
import pytest

from tests import mfcc_ref as R
from tests.test_gpu_extract_frontend import _extract, _model

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "tf_kaldi_speaker_amd")
LENS = {"utt_a": 16000, "utt_b": 24000, "utt_c": 48037, "utt_d": 8000, "utt_e": 32000, "utt_f": 20011}


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("make_mfcc")
    rs = np.random.RandomState(47)
    waves = {k: R.signal(rs, n, 16000.0) for k, n in LENS.items()}
    with open(str(tmp / "wav.scp"), "w") as scp:
        for k, x in waves.items():
            path = str(tmp / (k + ".wav"))
            with wave.open(path, "wb") as w:
                w.setnchannels(1)
                w.setsampwidth(2)
                w.setframerate(16000)
                w.writeframes(x.astype("<i2").tobytes())
            scp.write("%s %s\n" % (k, "cat %s |" % path if k == "utt_c" else path))
    (tmp / "mfcc.conf").write_text("--sample-frequency=16000\n--frame-length=25\n--low-freq=20\n--high-freq=7600\n--num-mel-bins=30\n--num-ceps=30\n"
                                   "--snip-edges=false\n")
    (tmp / "vad.conf").write_text("--vad-energy-threshold=5.5\n--vad-energy-mean-scale=0.5\n--vad-proportion-threshold=0.12\n--vad-frames-context=2\n")
    names = {n: str(tmp / n) for n in ("feats.ark", "feats.scp", "vad.ark", "vad.scp", "utt2num_frames")}
    env = dict(os.environ, TF_KALDI_ROOT=PKG, PYTHONPATH=PKG)
    r = subprocess.run([sys.executable, os.path.join(PKG, "nnet", "lib", "make_mfcc.py"), "--mfcc-config", str(tmp / "mfcc.conf"), "--vad-config",
                        str(tmp / "vad.conf"), "--compress", "true", "--write-utt2num-frames", names["utt2num_frames"], str(tmp / "wav.scp"),
                        "ark,scp:%s,%s" % (names["feats.ark"], names["feats.scp"]), "ark,scp:%s,%s" % (names["vad.ark"], names["vad.scp"])],
                       env=env, cwd=PKG, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    refs = {k: (R.mfcc(x, R.VOXCELEB), R.mfcc(x, R.VOXCELEB, np.float32)) for k, x in waves.items()}
    return tmp, names, waves, refs, r.stderr


def _mfcc_tolerance(r64, r32, cols):
    """tests/test_gpu_mfcc.py: 4 * D32 + 2^-21 |ref| per column class."""
    d32 = float(np.abs(r32[:, cols].astype(np.float64) - r64[:, cols]).max())
    return 4.0 * d32 + 2.0 ** -21 * np.abs(r64[:, cols])


def test_tables_keys_counts_and_vad(run):
    from tf_kaldi_speaker_amd.dataset import kaldi_io
    tmp, names, waves, refs, stderr = run
    assert "--dither=0" in stderr and "Computed features of 6 utterances" in stderr
    feats = list(kaldi_io.read_mat_scp(names["feats.scp"]))
    vads = list(kaldi_io.read_vec_flt_scp(names["vad.scp"]))
    assert [k for k, _ in feats] == [k for k, _ in vads] == list(LENS)                       # keys in order
    assert [k for k, _ in kaldi_io.read_mat_ark(names["feats.ark"])] == list(LENS)
    assert open(names["feats.ark"], "rb").read(11) == b"utt_a \0BCM "                        # --compress=true
    assert [ln.split() for ln in open(names["utt2num_frames"])] == [[k, str(R.num_frames(n, R.VOXCELEB))] for k, n in LENS.items()]
    for (k, got), (_, vad) in zip(feats, vads):
        r64 = refs[k][0]
        assert got.shape == r64.shape == (R.num_frames(LENS[k], R.VOXCELEB), 30) and vad.shape == (len(r64),) and vad.dtype == np.float32
        assert float(np.abs(r64[:, 0] - R.vad_threshold(r64[:, 0], 5.5, 0.5)).min()) > 1e-2
        assert np.array_equal(vad, R.energy_vad(r64, **R.VAD_VOXCELEB).astype(np.float32)), k
        assert "Key %s: %d samples, %d frames, %d voiced." % (k, LENS[k], len(r64), int(vad.sum())) in stderr


def test_archive_holds_the_kernel_features_through_the_codec(run):
    """What the archive holds is the 'CM ' codec's image of what the kernels give (misc.features.FeatureExtractor, in process), bit for bit,
    and those are within the MFCC tolerance of the restatement: the driver adds nothing but the codec."""
    from tf_kaldi_speaker_amd.dataset import kaldi_io
    from tf_kaldi_speaker_amd.misc import features
    tmp, names, waves, refs, _ = run
    fx = features.FeatureExtractor(features.MfccOptions.from_conf(str(tmp / "mfcc.conf")), features.VadOptions.from_conf(str(tmp / "vad.conf")),
                                   workspace_bytes=1 << 20)      # 1 MB: several batches
    direct = fx.extract([waves[k] for k in LENS])
    archive = dict(kaldi_io.read_mat_scp(names["feats.scp"]))
    for k, (x, _) in zip(LENS, direct):
        r64, r32 = refs[k]
        for cols in (slice(0, 1), slice(1, 30)):
            assert (np.abs(x[:, cols].astype(np.float64) - r64[:, cols]) <= _mfcc_tolerance(r64, r32, cols)).all(), k
        buf = io.BytesIO()
        kaldi_io.write_compressed_mat(buf, x, key=k, header="uniform")
        buf.seek(0)
        assert np.array_equal(dict(kaldi_io.read_mat_ark(buf))[k].view(np.uint32), archive[k].view(np.uint32)), k


def test_features_within_mfcc_tolerance_plus_cm_step(run):
    """|archive - ref| <= MFCC tolerance + (max - min) / 255 of the column.  The driver writes 'CM ' matrices with evenly spaced header points
    (kaldi_io.write_compressed_mat, header="uniform"): 64 / 128 / 63 codes over a quarter / half / quarter of the column's range, a rounding
    error of at most (max - min) / 504 plus what the header's uint16 grid adds.  With Kaldi's quartile points the same format is off by up to
    (max - min) / 126 where an outer quarter of the values spans most of the range - 1.13 ... 1.98 of the step on these six utterances, on the
    fp64 restatement alone - which is why the driver does not use them."""
    from tf_kaldi_speaker_amd.dataset import kaldi_io
    tmp, names, waves, refs, _ = run
    worst = 0.0
    for k, got in kaldi_io.read_mat_scp(names["feats.scp"]):
        r64, r32 = refs[k]
        step = (r64.max(axis=0) - r64.min(axis=0)) / 255.0
        for cols in (slice(0, 1), slice(1, 30)):
            tol = _mfcc_tolerance(r64, r32, cols) + step[None, cols]
            ratio = float((np.abs(got[:, cols].astype(np.float64) - r64[:, cols]) / tol).max())
            print("%s columns %s: worst error / (MFCC tolerance + CM step) %.3f" % (k, cols, ratio))
            worst = max(worst, ratio)
    assert worst <= 1.0, worst


def test_extract_accepts_the_two_tables(run, tmp_path):
    from tf_kaldi_speaker_amd.dataset import kaldi_io
    _, names, _, _, _ = run
    model = str(tmp_path / "exp")
    _model(model).close()
    out = str(tmp_path / "xvector.ark")
    err = _extract(["--cmn-window", "300", "--vad", "scp:" + names["vad.scp"], "--chunk-size", "10000", "--min-chunk-size", "25", model,
                    "ark:" + names["feats.ark"], "ark:" + out])
    vectors = list(kaldi_io.read_vec_flt_ark(out))
    assert [k for k, _ in vectors] == list(LENS), err[-2000:]
    assert all(v.shape == (512,) and np.isfinite(v).all() and np.abs(v).max() > 0 for _, v in vectors)
