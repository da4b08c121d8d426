"""nnet/lib/augment.py and nnet/lib/make_mfcc.py --augment-plan on a real MI355X: six synthetic wavs, two impulse responses and two noises
in a tmp dir under a plan that covers the four lists of the recipe (reverb, noise, music, babble) plus a mixed and a clean line.
  - augment.py writes wavs that read_wav reads back equal to Augmenter's arrays, and those sit within one PCM step of the fp64 restatement;
  - make_mfcc.py --augment-plan writes archives equal BYTE FOR BYTE to make_mfcc.py run on augment.py's wav.scp: the same PCM in gives the
    same features out, with no wav file in between;
  - those features are within the MFCC tolerance plus the codec step (tests/test_gpu_make_mfcc.py) of the MFCC restatement of the kernel's
    own PCM (a +-1 truncation difference against the augmentation restatement would otherwise enter);
  - make_mfcc.py without the new options (the run on augment.py's wav.scp is one) writes what FeatureExtractor.extract gives, through the codec,
    bit for bit.
The drivers run once for the module."""
import io
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import augment_ref as A
from tests import mfcc_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "tf_kaldi_speaker_amd")
LENS = {"utt_a": 16000, "utt_b": 24000, "utt_c": 20011, "utt_d": 8000, "utt_e": 32000, "utt_f": 12345}
RIRS = {"room1": (2000, 37), "room2": (801, 0)}
NOISES = {"hum": 8000, "street": 20011}
PLAN = ("utt_a-reverb utt_a rir=room1\n"
        "utt_a-reverb2 utt_a rir=room2\n"
        "utt_b-noise utt_b noise=hum:15:0 noise=street:5:0.75 noise=hum:0:1.4\n"
        "utt_c-music utt_c noise=street:8:0:bg\n"
        "utt_d-babble utt_d noise=hum:20:0:bg noise=street:17:0:bg noise=hum:13:0:bg\n"
        "utt_e-mixed utt_e rir=room2 noise=street:10:0:bg noise=hum:5:1.0\n"
        "utt_f-clean utt_f\n")


def _driver(name, argv):
    env = dict(os.environ, TF_KALDI_ROOT=PKG, PYTHONPATH=PKG)
    r = subprocess.run([sys.executable, os.path.join(PKG, "nnet", "lib", name)] + argv, env=env, cwd=PKG, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stderr


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    from tf_kaldi_speaker_amd.misc import augment
    tmp = tmp_path_factory.mktemp("augment")
    rs = np.random.RandomState(83)
    waves = {k: A.signal(rs, n) for k, n in LENS.items()}
    rirs = {k: A.rir(rs, L, p) for k, (L, p) in RIRS.items()}
    noises = {k: A.signal(rs, n) for k, n in NOISES.items()}
    for name, table in (("wav", waves), ("rir", rirs), ("noise", noises)):
        with open(str(tmp / (name + ".scp")), "w") as scp:
            for k, x in table.items():
                path = str(tmp / ("%s_%s.wav" % (name, k)))
                augment.write_wav(path, x, 16000.0)
                scp.write("%s %s\n" % (k, "cat %s |" % path if k == "utt_c" else path))
    (tmp / "plan").write_text(PLAN)
    (tmp / "mfcc.conf").write_text("--sample-frequency=16000\n--frame-length=25\n--low-freq=20\n--high-freq=7600\n--num-mel-bins=30\n--num-ceps=30\n"
                                   "--snip-edges=false\n")
    (tmp / "augment.conf").write_text("--shift-output=true\n--normalize-output=true\n")
    tables = ["--rir-scp", str(tmp / "rir.scp"), "--noise-scp", str(tmp / "noise.scp")]
    out_dir = str(tmp / "augmented")
    log_aug = _driver("augment.py", ["--config", str(tmp / "augment.conf")] + tables + [str(tmp / "plan"), str(tmp / "wav.scp"), out_dir])
    names = {}
    for tag in ("direct", "files"):
        names[tag] = {n: str(tmp / ("%s_%s" % (tag, n))) for n in ("feats.ark", "feats.scp", "vad.ark", "vad.scp")}
    spec = lambda t: ["ark,scp:%s,%s" % (names[t]["feats.ark"], names[t]["feats.scp"]), "ark,scp:%s,%s" % (names[t]["vad.ark"], names[t]["vad.scp"])]
    log_direct = _driver("make_mfcc.py", ["--mfcc-config", str(tmp / "mfcc.conf"), "--augment-plan", str(tmp / "plan"), "--augment-config",
                                          str(tmp / "augment.conf")] + tables + [str(tmp / "wav.scp")] + spec("direct"))
    log_files = _driver("make_mfcc.py", ["--mfcc-config", str(tmp / "mfcc.conf"), os.path.join(out_dir, "wav.scp")] + spec("files"))
    entries = augment.read_plan(str(tmp / "plan"), 16000.0, rirs, noises)
    return dict(tmp=tmp, waves=waves, rirs=rirs, noises=noises, out_dir=out_dir, names=names, entries=entries,
                logs=dict(augment=log_aug, direct=log_direct, files=log_files))


def _written(run):
    from tf_kaldi_speaker_amd.misc import augment, features
    return {k: features.read_wav(rx, features.MfccOptions(), k) for k, rx in augment.read_scp(os.path.join(run["out_dir"], "wav.scp"))}


def test_augment_writes_what_the_augmenter_gives(run):
    from tf_kaldi_speaker_amd.misc import augment
    entries = run["entries"]
    written = _written(run)
    assert list(written) == [e.out_key for e in entries] == [ln.split()[0] for ln in PLAN.splitlines()]
    aug = augment.Augmenter(augment.AugmentOptions(), run["rirs"], run["noises"], 16000.0, workspace_bytes=1 << 20)      # 1 MB: several calls
    arrays, clipped = aug.augment([run["waves"][e.src_key] for e in entries], entries)
    for e, got, c in zip(entries, arrays, clipped):
        assert got.dtype == np.int16 and np.array_equal(written[e.out_key], got), e.out_key
        assert len(got) == LENS[e.src_key]                                                       # --shift-output=true: the source's length
        assert "Key %s: %d samples, rir %s, %d noises, %d clipped." % (e.out_key, len(got), e.rir or "-", len(e.noises), c) in run["logs"]["augment"]
        noises = [(run["noises"][nid], snr, start, "bg" if bg else None) for nid, snr, start, bg in e.noises]
        ref = A.augment(run["waves"][e.src_key], run["rirs"][e.rir] if e.rir else None, noises)
        q, count = A.quantise(ref)
        assert count == 0 == c and np.abs(q.astype(np.int32) - got.astype(np.int32)).max() <= 1, e.out_key
        print("%s: %d of %d samples one PCM step from the restatement" % (e.out_key, int((q != got).sum()), len(got)))
    assert np.array_equal(written["utt_f-clean"], run["waves"]["utt_f"])                      # nothing to add: the source itself
    assert "Augmented 7 utterances" in run["logs"]["augment"]
    with pytest.raises(ValueError, match="does not hold utterance 0"):
        list(augment.Augmenter(augment.AugmentOptions(), run["rirs"], run["noises"], 16000.0, workspace_bytes=1 << 10).run(
            [run["waves"]["utt_a"]], entries[:1]))


def test_make_mfcc_with_a_plan_equals_make_mfcc_on_the_written_wavs(run):
    names = run["names"]
    for n in ("feats.ark", "vad.ark"):
        a, b = open(names["direct"][n], "rb").read(), open(names["files"][n], "rb").read()
        assert len(a) > 1000 and a == b, n
    keys = [e.out_key for e in run["entries"]]
    for tag in ("direct", "files"):
        assert [ln.split()[0] for ln in open(names[tag]["feats.scp"])] == keys == [ln.split()[0] for ln in open(names[tag]["vad.scp"])]
        assert "Computed features of 7 utterances" in run["logs"][tag]
    assert "Key utt_e-mixed: augmented from utt_e, rir room2, 2 noises, 0 clipped." in run["logs"]["direct"]
    assert "augmented from" not in run["logs"]["files"]


def test_features_match_the_restatement_of_the_kernel_pcm_and_the_plain_driver_is_unchanged(run):
    from tf_kaldi_speaker_amd.dataset import kaldi_io
    from tf_kaldi_speaker_amd.misc import features
    written = _written(run)
    archive = dict(kaldi_io.read_mat_scp(run["names"]["direct"]["feats.scp"]))
    vads = dict(kaldi_io.read_vec_flt_scp(run["names"]["direct"]["vad.scp"]))
    fx = features.FeatureExtractor(features.MfccOptions.from_conf(str(run["tmp"] / "mfcc.conf")), features.VadOptions())
    direct = fx.extract([written[k] for k in written])
    worst = 0.0
    for (k, pcm), (x, decisions) in zip(written.items(), direct):
        buf = io.BytesIO()
        kaldi_io.write_compressed_mat(buf, x, key=k, header="uniform")
        buf.seek(0)
        assert np.array_equal(dict(kaldi_io.read_mat_ark(buf))[k].view(np.uint32), archive[k].view(np.uint32)), k      # the plain driver: extract + codec
        assert np.array_equal(vads[k], decisions), k
        r64, r32 = R.mfcc(pcm, R.VOXCELEB), R.mfcc(pcm, R.VOXCELEB, np.float32)
        assert archive[k].shape == r64.shape
        step = (r64.max(axis=0) - r64.min(axis=0)) / 255.0
        for cols in (slice(0, 1), slice(1, 30)):
            d32 = float(np.abs(r32[:, cols].astype(np.float64) - r64[:, cols]).max())
            tol = 4.0 * d32 + 2.0 ** -21 * np.abs(r64[:, cols]) + step[None, cols]
            ratio = float((np.abs(archive[k][:, cols].astype(np.float64) - r64[:, cols]) / tol).max())
            print("%s columns %s: worst error / (MFCC tolerance + CM step) %.3f" % (k, cols, ratio))
            worst = max(worst, ratio)
    assert worst <= 1.0, worst
