#!/usr/bin/env python3
"""Wall time of extract.py's wav mode against the two-step path it replaces, on a synthetic wav.scp - a diagnostic, not a test:

    python tools/bench_extract_wav.py [files=512] > profiles/extract_wav_bench.txt

files 16 kHz recordings of 4 - 12 s (tones + noise with quiet stretches, as tools/bench_kernel.py mfcc) are written to a temporary
directory with a toy x-vector model (tests/test_gpu_extract_frontend.py builds it).  Timed, each as its own process, wall clock:
  two-step   make_mfcc.py (--compress true, the default, and false) -> feats.ark, vad.scp; extract.py --cmn-window 300 --vad scp:
  wav mode   extract.py --mfcc-config --vad-config --cmn-window 300 wav.scp
and, in this process, the two halves of the wav mode's work: reading the files (misc.features.read_wav_scp: the stdlib wave module) and
the device chain on the samples already in memory (upload, xv_mfcc, xv_energy_vad, one count per utterance back).  A process pays ~5 s of
start-up (torch, the library, the model) whatever it does; the drivers' own "in X s" lines exclude it."""
import os
import re
import subprocess
import sys
import tempfile
import time
import wave

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "tf_kaldi_speaker_amd")
sys.path.insert(0, ROOT)
import numpy as np


def run(script, args):
    env = dict(os.environ, TF_KALDI_ROOT=PKG, PYTHONPATH=PKG)
    t0 = time.time()
    r = subprocess.run([sys.executable, os.path.join(PKG, "nnet", "lib", script)] + args, env=env, cwd=PKG, capture_output=True, text=True)
    wall = time.time() - t0
    if r.returncode != 0:
        sys.exit(r.stderr[-3000:])
    own = re.findall(r"\[INFO\] (?:Extracted|Computed features of) .*", r.stderr)
    return wall, own[-1] if own else ""


def main():
    import torch
    from tests.test_gpu_extract_frontend import _model
    from tf_kaldi_speaker_amd.misc import features
    n_files = int(sys.argv[1]) if len(sys.argv) > 1 else 512
    rs = np.random.RandomState(0)
    sf = 16000
    with tempfile.TemporaryDirectory() as tmp:
        lens = rs.randint(4 * sf, 12 * sf + 1, n_files)
        t = np.arange(int(lens.max())) / float(sf)
        tone = 3000.0 * np.sin(2.0 * np.pi * 220.0 * t) + 1500.0 * np.sin(2.0 * np.pi * 1830.0 * t)
        gate = np.where(np.floor(t / 0.25).astype(np.int64) % 3 == 2, 0.02, 1.0)
        with open(os.path.join(tmp, "wav.scp"), "w") as scp:
            for i, n in enumerate(lens):
                path = os.path.join(tmp, "utt%04d.wav" % i)
                with wave.open(path, "wb") as w:
                    w.setnchannels(1)
                    w.setsampwidth(2)
                    w.setframerate(sf)
                    w.writeframes(np.rint(tone[:n] * gate[:n] + rs.randn(n) * 40.0).astype("<i2").tobytes())
                scp.write("utt%04d %s\n" % (i, path))
        mfcc, vad, scp = (os.path.join(tmp, n) for n in ("mfcc.conf", "vad.conf", "wav.scp"))
        open(mfcc, "w").write("--sample-frequency=16000\n--frame-length=25\n--low-freq=20\n--high-freq=7600\n--num-mel-bins=30\n--num-ceps=30\n--snip-edges=false\n")
        open(vad, "w").write("--vad-energy-threshold=5.5\n--vad-energy-mean-scale=0.5\n--vad-proportion-threshold=0.12\n--vad-frames-context=2\n")
        model = os.path.join(tmp, "exp")
        _model(model).close()
        print("%d files of %.1f - %.1f s at 16 kHz, %.1f M samples (%.0f MB of RIFF PCM-16); toy tdnn, --cmn-window 300, VoxCeleb mfcc.conf / vad.conf"
              % (n_files, lens.min() / sf, lens.max() / sf, lens.sum() / 1e6, 2.0 * lens.sum() / 1e6), flush=True)
        common = ["--cmn-window", "300", "--min-chunk-size", "25", "--chunk-size", "10000"]
        for compress in ("true", "false"):
            feats, vads = os.path.join(tmp, "feats_%s.ark" % compress), os.path.join(tmp, "vad_%s" % compress)
            w1, own1 = run("make_mfcc.py", ["--mfcc-config", mfcc, "--vad-config", vad, "--compress", compress, scp, "ark:" + feats,
                                            "ark,scp:%s.ark,%s.scp" % (vads, vads)])
            w2, own2 = run("extract.py", common + ["--vad", "scp:%s.scp" % vads, model, "ark:" + feats, "ark:" + os.path.join(tmp, "two_%s.ark" % compress)])
            print("two-step, --compress %-5s  wall %6.2f s = make_mfcc.py %6.2f s + extract.py %6.2f s   (%.0f MB of features on disk)"
                  % (compress, w1 + w2, w1, w2, os.path.getsize(feats) / 1e6), flush=True)
            print("    %s\n    %s" % (own1, own2), flush=True)
        w3, own3 = run("extract.py", common + ["--mfcc-config", mfcc, "--vad-config", vad, model, scp, "ark:" + os.path.join(tmp, "wav.ark")])
        print("wav mode                   wall %6.2f s = extract.py alone\n    %s" % (w3, own3), flush=True)
        same = open(os.path.join(tmp, "wav.ark"), "rb").read() == open(os.path.join(tmp, "two_false.ark"), "rb").read()
        print("wav mode's embeddings are %s those of the two-step path with --compress false" % ("bit for bit" if same else "NOT bit for bit"), flush=True)
        # the two halves of the wav mode's own work, in this process
        options = features.MfccOptions.from_conf(mfcc)
        t0 = time.time()
        waves = [w for _, w, _ in features.read_wav_scp(scp, options)]
        t_read = time.time() - t0
        fx = features.FeatureExtractor(options, features.VadOptions.from_conf(vad), "cuda:0")
        rates = [sf] * len(waves)
        for _ in fx.device_batches(waves[:8], rates[:8]):      # warm: the first launch loads the code object
            pass
        torch.cuda.synchronize()
        t0 = time.time()
        kept = sum(sum(batch.kept) for _, _, batch in fx.device_batches(waves, rates))
        torch.cuda.synchronize()
        t_dev = time.time() - t0
        print("in process: reading the %d files (stdlib wave) %.3f s = %.0f MB/s; upload + xv_mfcc + xv_energy_vad + the kept counts back %.3f s (%d frames kept)"
              % (n_files, t_read, 2.0 * lens.sum() / 1e6 / t_read, t_dev, kept), flush=True)


if __name__ == "__main__":
    main()
