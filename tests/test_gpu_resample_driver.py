"""nnet/lib/resample.py and the resampling paths of make_mfcc.py and augment.py on a real MI355X: a few synthetic wavs of at most 2 s in a
tmp dir.
  - resample.py --to-rate 8000 writes what Resampler.resample returns;
  - make_mfcc.py with an 8 kHz conf plus --allow-downsample=true on the 16 kHz wavs writes archives equal BYTE FOR BYTE to make_mfcc.py on
    resample.py's wavs, and those features are within the MFCC tolerance plus the codec step (tests/test_gpu_augment_driver.py) of the MFCC
    restatement of the kernel's own PCM;
  - augment.py --resample-signals true with 16 kHz impulse responses and noises against 8 kHz sources writes the bytes augment.py writes
    when it is given the files resample.py made from them;
  - a plan line `speed=0.9 rir=... noise=...` gives the bytes of augmenting resample.py --speed 0.9's output with the line minus speed=;
  - a speed=1.1 copy has ceil(n * 10 / 11) samples, at most one PCM step from rint-and-clamp of the fp64 restatement, and differs from it
    only where the fp64 value lies within the fp32 tolerance of a half.
The drivers run once for the module."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import augment_ref as A
from tests import mfcc_ref as M
from tests import resample_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "tf_kaldi_speaker_amd")
LENS = {"utt_a": 16000, "utt_b": 22011, "utt_c": 8000, "utt_d": 32000}
RIRS = {"room1": (1201, 37), "room2": (801, 0)}
NOISES = {"hum": 8000, "street": 20011}
PLAN_8K = ("utt_a-reverb utt_a rir=room1\n"
           "utt_b-noise utt_b noise=hum:15:0 noise=street:5:0.75\n"
           "utt_d-mixed utt_d rir=room2 noise=street:10:0:bg noise=hum:5:1.0\n")
PLAN_SPEED = ("utt_a-slow utt_a speed=0.9 rir=room1 noise=hum:10:0:bg\n"
              "utt_c-slow utt_c speed=0.9 noise=street:8:0.25\n")
PLAN_FAST = "sp1.1-utt_b utt_b speed=1.1\n"


def _driver(name, argv):
    env = dict(os.environ, TF_KALDI_ROOT=PKG, PYTHONPATH=PKG)
    r = subprocess.run([sys.executable, os.path.join(PKG, "nnet", "lib", name)] + argv, env=env, cwd=PKG, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stderr


def _wavs(scp, rate):
    from tf_kaldi_speaker_amd.misc import augment, features
    return {k: features.read_wav(rx, features.MfccOptions(sample_frequency=float(rate)), k) for k, rx in augment.read_scp(scp)}


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    from tf_kaldi_speaker_amd.misc import augment
    tmp = tmp_path_factory.mktemp("resample")
    rs = np.random.RandomState(29)
    waves = {k: A.signal(rs, n) for k, n in LENS.items()}
    rirs = {k: A.rir(rs, L, p) for k, (L, p) in RIRS.items()}
    noises = {k: A.signal(rs, n) for k, n in NOISES.items()}
    for name, table in (("wav", waves), ("rir", rirs), ("noise", noises)):
        with open(str(tmp / (name + ".scp")), "w") as scp:
            for k, x in table.items():
                path = str(tmp / ("%s_%s.wav" % (name, k)))
                augment.write_wav(path, x, 16000.0)
                scp.write("%s %s\n" % (k, "cat %s |" % path if k == "utt_c" else path))
    p = lambda name: str(tmp / name)
    (tmp / "signals.scp").write_text(open(p("rir.scp")).read() + open(p("noise.scp")).read())
    (tmp / "plan8").write_text(PLAN_8K)
    (tmp / "plan_speed").write_text(PLAN_SPEED + PLAN_FAST)
    (tmp / "plan_plain").write_text(PLAN_SPEED.replace(" speed=0.9", ""))
    sre = "--sample-frequency=8000\n--frame-length=25\n--low-freq=20\n--high-freq=3700\n--num-mel-bins=23\n--num-ceps=23\n--snip-edges=false\n"
    (tmp / "mfcc8.conf").write_text(sre)
    (tmp / "mfcc8_allow.conf").write_text(sre + "--allow-downsample=true\n")
    logs = {}
    logs["to8"] = _driver("resample.py", ["--to-rate", "8000", p("wav.scp"), p("wav8")])
    logs["signals8"] = _driver("resample.py", ["--to-rate", "8000", p("signals.scp"), p("signals8")])
    logs["slow"] = _driver("resample.py", ["--speed", "0.9", p("wav.scp"), p("slow")])
    made = dict(ln.split(None, 1) for ln in open(os.path.join(p("signals8"), "wav.scp")))
    for name, table in (("rir8", rirs), ("noise8", noises)):
        (tmp / (name + ".scp")).write_text("".join("%s %s" % (k, made[k]) for k in table))
    names = {tag: {n: p("%s_%s" % (tag, n)) for n in ("feats.ark", "feats.scp", "vad.ark", "vad.scp")} for tag in ("direct", "files")}
    spec = lambda t: ["ark,scp:%s,%s" % (names[t]["feats.ark"], names[t]["feats.scp"]), "ark,scp:%s,%s" % (names[t]["vad.ark"], names[t]["vad.scp"])]
    logs["direct"] = _driver("make_mfcc.py", ["--mfcc-config", p("mfcc8_allow.conf"), p("wav.scp")] + spec("direct"))
    logs["files"] = _driver("make_mfcc.py", ["--mfcc-config", p("mfcc8.conf"), os.path.join(p("wav8"), "wav.scp")] + spec("files"))
    wav8 = os.path.join(p("wav8"), "wav.scp")
    logs["aug_signals"] = _driver("augment.py", ["--sample-frequency", "8000", "--resample-signals", "true", "--rir-scp", p("rir.scp"), "--noise-scp",
                                                 p("noise.scp"), p("plan8"), wav8, p("aug_signals")])
    logs["aug_files"] = _driver("augment.py", ["--sample-frequency", "8000", "--rir-scp", p("rir8.scp"), "--noise-scp", p("noise8.scp"), p("plan8"), wav8,
                                               p("aug_files")])
    tables = ["--rir-scp", p("rir.scp"), "--noise-scp", p("noise.scp")]
    logs["aug_speed"] = _driver("augment.py", tables + [p("plan_speed"), p("wav.scp"), p("aug_speed")])
    logs["aug_plain"] = _driver("augment.py", tables + [p("plan_plain"), os.path.join(p("slow"), "wav.scp"), p("aug_plain")])
    return dict(tmp=tmp, p=p, waves=waves, rirs=rirs, noises=noises, names=names, logs=logs)


def test_resample_writes_what_the_resampler_gives(run):
    from tf_kaldi_speaker_amd.misc import resample
    written = _wavs(os.path.join(run["p"]("wav8"), "wav.scp"), 8000)
    assert list(written) == list(LENS)
    rs = resample.Resampler(16000, 8000, workspace_bytes=1 << 17)      # 128 KB: several calls
    arrays, clipped = rs.resample([run["waves"][k] for k in LENS])
    plan = R.Plan(16000, 8000)
    for k, got, c in zip(LENS, arrays, clipped):
        assert got.dtype == np.int16 and np.array_equal(written[k], got), k
        assert len(got) == plan.num_samples(LENS[k]) and c == 0
        assert "Key %s: %d samples at 16000 Hz -> %d samples at 8000 Hz, 0 clipped." % (k, LENS[k], len(got)) in run["logs"]["to8"]
        q, count = R.quantise(R.resample(run["waves"][k], plan))
        assert count == 0 and np.abs(q.astype(np.int32) - got.astype(np.int32)).max() <= 1, k
    assert "Resampled 4 utterances" in run["logs"]["to8"]
    with pytest.raises(ValueError, match="does not hold utterance 0"):
        resample.Resampler(16000, 8000, workspace_bytes=1 << 10).run([run["waves"]["utt_a"]])
    # --speed keeps the rate: 0.9 at 16 kHz is 14400 -> 16000
    slow = _wavs(os.path.join(run["p"]("slow"), "wav.scp"), 16000)
    arrays, _ = resample.Resampler(*resample.speed_rates("0.9", 16000)).resample([run["waves"][k] for k in LENS])
    for k, got in zip(LENS, arrays):
        assert np.array_equal(slow[k], got) and len(got) == -(-LENS[k] * 10 // 9), k


def test_make_mfcc_allow_downsample_equals_make_mfcc_on_the_resampled_wavs(run):
    from tf_kaldi_speaker_amd.dataset import kaldi_io
    names = run["names"]
    for n in ("feats.ark", "vad.ark"):
        a, b = open(names["direct"][n], "rb").read(), open(names["files"][n], "rb").read()
        assert len(a) > 1000 and a == b, n
    for tag in ("direct", "files"):
        assert [ln.split()[0] for ln in open(names[tag]["feats.scp"])] == list(LENS)
        assert "Computed features of 4 utterances" in run["logs"][tag]
    assert "Key utt_b: resampled from 16000 Hz." in run["logs"]["direct"] and "resampled from" not in run["logs"]["files"]
    # without the switch the refusal stays
    env = dict(os.environ, TF_KALDI_ROOT=PKG, PYTHONPATH=PKG)
    r = subprocess.run([sys.executable, os.path.join(PKG, "nnet", "lib", "make_mfcc.py"), "--mfcc-config", run["p"]("mfcc8.conf"), run["p"]("wav.scp"),
                        "ark:" + run["p"]("refused.ark"), "ark:" + run["p"]("refused_vad.ark")], env=env, cwd=PKG, capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "no resampling" in r.stderr and "--allow-downsample=true" in r.stderr, r.stderr[-2000:]
    written = _wavs(os.path.join(run["p"]("wav8"), "wav.scp"), 8000)
    archive = dict(kaldi_io.read_mat_scp(names["direct"]["feats.scp"]))
    worst = 0.0
    for k, pcm in written.items():
        r64, r32 = M.mfcc(pcm, M.SRE), M.mfcc(pcm, M.SRE, np.float32)
        assert archive[k].shape == r64.shape
        step = (r64.max(axis=0) - r64.min(axis=0)) / 255.0
        for cols in (slice(0, 1), slice(1, 23)):
            d32 = float(np.abs(r32[:, cols].astype(np.float64) - r64[:, cols]).max())
            tol = 4.0 * d32 + 2.0 ** -21 * np.abs(r64[:, cols]) + step[None, cols]
            ratio = float((np.abs(archive[k][:, cols].astype(np.float64) - r64[:, cols]) / tol).max())
            print("%s columns %s: worst error / (MFCC tolerance + CM step) %.3f" % (k, cols, ratio))
            worst = max(worst, ratio)
    assert worst <= 1.0, worst


def _same_wavs(run, a, b, rate, keys):
    x, y = _wavs(os.path.join(run["p"](a), "wav.scp"), rate), _wavs(os.path.join(run["p"](b), "wav.scp"), rate)
    assert list(x) == list(y) == keys
    for k in keys:
        assert len(x[k]) > 1000 and np.array_equal(x[k], y[k]), k
        assert open(os.path.join(run["p"](a), "wav", k + ".wav"), "rb").read() == open(os.path.join(run["p"](b), "wav", k + ".wav"), "rb").read(), k
    return x


def test_augment_resample_signals_equals_augment_on_the_resampled_files(run):
    out = _same_wavs(run, "aug_signals", "aug_files", 8000, [ln.split()[0] for ln in PLAN_8K.splitlines()])
    plan = R.Plan(16000, 8000)
    assert len(out["utt_a-reverb"]) == plan.num_samples(LENS["utt_a"])      # --shift-output=true: the 8 kHz source's length
    # without the switch the refusal stays
    env = dict(os.environ, TF_KALDI_ROOT=PKG, PYTHONPATH=PKG)
    r = subprocess.run([sys.executable, os.path.join(PKG, "nnet", "lib", "augment.py"), "--sample-frequency", "8000", "--rir-scp", run["p"]("rir.scp"),
                        run["p"]("plan8"), os.path.join(run["p"]("wav8"), "wav.scp"), run["p"]("refused")], env=env, cwd=PKG, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode != 0 and "no resampling" in r.stderr, r.stderr[-2000:]


def test_speed_in_the_plan_equals_augmenting_the_perturbed_wavs(run):
    keys = [ln.split()[0] for ln in PLAN_SPEED.splitlines()]
    x = _wavs(os.path.join(run["p"]("aug_speed"), "wav.scp"), 16000)
    y = _wavs(os.path.join(run["p"]("aug_plain"), "wav.scp"), 16000)
    assert list(x) == keys + ["sp1.1-utt_b"] and list(y) == keys
    for k, src in zip(keys, ("utt_a", "utt_c")):
        assert np.array_equal(x[k], y[k]) and len(x[k]) == -(-LENS[src] * 10 // 9), k
        assert open(os.path.join(run["p"]("aug_speed"), "wav", k + ".wav"), "rb").read() == open(os.path.join(run["p"]("aug_plain"), "wav", k + ".wav"), "rb").read()
    assert "Key utt_a-slow: %d samples, speed 0.9, rir room1, 1 noises, " % len(x["utt_a-slow"]) in run["logs"]["aug_speed"]


def test_a_speed_1_1_copy_sits_on_the_restatement(run):
    got = _wavs(os.path.join(run["p"]("aug_speed"), "wav.scp"), 16000)["sp1.1-utt_b"]
    n = LENS["utt_b"]
    assert len(got) == -(-n * 10 // 11)
    plan = R.Plan(17600, 16000)
    # nothing is added to the copy, but --normalize-output scales y by sqrt(P0 / Pa) with P0 = Pa: 1.0 exactly
    r64 = R.resample(run["waves"]["utt_b"], plan)
    r32 = R.resample(run["waves"]["utt_b"], plan, np.float32)
    q, count = R.quantise(r64)
    assert count == 0 and len(q) == len(got)
    diff = q.astype(np.int32) - got.astype(np.int32)
    assert np.abs(diff).max() <= 1
    tol = 4.0 * float(np.abs(r32.astype(np.float64) - r64).max()) + 2.0 ** -21 * np.abs(r64)
    half = np.abs(np.abs(r64 - np.floor(r64)) - 0.5)
    print("sp1.1-utt_b: %d of %d samples one PCM step from the restatement" % (int((diff != 0).sum()), len(got)))
    assert (half[diff != 0] <= tol[diff != 0]).all()
