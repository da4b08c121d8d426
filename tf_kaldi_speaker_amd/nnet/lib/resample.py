#!/usr/bin/env python3
"""Sample-rate conversion or speed perturbation of a wav.scp on the GPU:

    python nnet/lib/resample.py [-g GPU] [--to-rate HZ | --speed F] [--channel C] wav.scp out_dir

What the `sox -r 8k` stages of the 8 kHz recipes do to every impulse response and MUSAN file (egs/sre/v1/local/make_musan.sh,
run.sh:135-142: reverberate_data_dir.py --source-sampling-rate 8000), and the 0.9 / 1.1 copies of x-vector training.  wav.scp: `key
rxfilename` lines, the rxfilename a RIFF PCM-16 file or a `command |` that writes one; the files may have different rates.
--to-rate HZ: every file comes out at HZ (a file that has it already is copied).  --speed F: every file is resampled F * rate -> rate and
keeps its rate - 0.9 makes it longer and lower; F * rate must be a whole number and F lie in 0.5 .. 2.  Writes out_dir/wav/<key>.wav (mono
RIFF PCM-16, rounded to nearest) and out_dir/wav.scp, and logs per key its samples and clipped samples.  The files are grouped by their
rate: one table per conversion.  The arithmetic is Kaldi's LinearResample with ResampleWaveform's cutoff as include/xvector_hip.h
restates it - not sox's resampler and not `sox speed`'s.
"""
import sys
import time

import _cli
from misc import resample, waves

# samples converted together (Resampler cuts them into calls that fit its workspace)
WINDOW_UTTERANCES = 256
WINDOW_SAMPLES = 64 << 20


def main():
    log = _cli.logger()
    args = _cli.parser_for("gpu", "to_rate", "speed", "channel", "wav_scp", "resample_out_dir").parse_args()
    if bool(args.to_rate) == bool(args.speed):
        sys.exit("one of --to-rate HZ and --speed F is needed")
    if args.to_rate < 0:
        sys.exit("--to-rate=%d: a sample rate of at least 1 Hz is expected" % args.to_rate)
    try:
        wavs = waves.read_scp(args.wav_scp)
    except ValueError as e:
        sys.exit(str(e))
    device = _cli.device(args.gpu)
    any_rate = waves.WavFormat(channel=args.channel)
    out_dir = waves.WavDir(args.out_dir)
    resamplers = waves.Resamplers(device)
    stats = {"utts": 0, "samples": 0, "clipped": 0, "t0": time.time()}
    windows = {}      # source rate -> [(key, samples)]
    done = {}         # key -> its line of wav.scp, written in the order of the input

    def flush(rate):
        window = windows.pop(rate, [])
        if not window:
            return
        try:
            fin, fout = (rate, args.to_rate) if args.to_rate else resample.speed_rates(args.speed, rate)
        except ValueError as e:
            sys.exit("Key %s: %s" % (window[0][0], e))
        if fin == fout:
            outs, clipped = [w for _, w in window], [0] * len(window)
        else:
            try:
                resampler = resamplers[fin, fout]
            except Exception as e:      # a conversion the library refuses by name (a table that does not fit)
                sys.exit("Key %s: %s" % (window[0][0], e))
            outs, clipped = resampler.resample([w for _, w in window])
        for (key, w), out, c in zip(window, outs, clipped):
            done[key] = out_dir.write(key, out, fout)
            log.info("[INFO] Key %s: %d samples at %d Hz -> %d samples at %d Hz, %d clipped." % (key, len(w), rate, len(out), fout, int(c)))
            stats["utts"] += 1
            stats["samples"] += len(out)
            stats["clipped"] += int(c)

    for key, rx in wavs:
        if key in done or any(key == k for w in windows.values() for k, _ in w):
            sys.exit("%s: key %s is listed twice" % (args.wav_scp, key))
        try:
            samples, rate = waves.read_wav_rate(rx, any_rate, key, any_rate=True)
        except ValueError as e:
            sys.exit(str(e))
        window = windows.setdefault(rate, [])
        window.append((key, samples))
        if len(window) >= WINDOW_UTTERANCES or sum(len(w) for _, w in window) >= WINDOW_SAMPLES:
            flush(rate)
    for rate in sorted(windows):
        flush(rate)
    with open(out_dir.scp_path, "w") as scp:
        scp.writelines(done[key] for key, _ in wavs)
    log.info("[INFO] Resampled %d utterances (%d samples, %d clipped) in %.2f s." % (stats["utts"], stats["samples"], stats["clipped"],
                                                                                    time.time() - stats["t0"]))


if __name__ == "__main__":
    main()
