#!/usr/bin/env python3
"""Reverberated and noisy copies of a wav.scp on the GPU:

    python nnet/lib/augment.py [-g GPU] [--config conf/augment.conf] [--sample-frequency 16000] [--resample-signals true]
                               --rir-scp rir.scp --noise-scp noise.scp plan wav.scp out_dir
    python nnet/lib/augment.py --make-plan {reverb,noise,music,babble} [--seed N] [--fg-interval S] --rir-scp rir.scp --noise-scp noise.scp
                               plan wav.scp
    python nnet/lib/augment.py --make-speed-plan 0.9,1.1 plan wav.scp

The augmentation stage of the recipe, for which the reference goes to Kaldi (egs/voxceleb/v1/run.sh:68-130: the reverberated, noise, music
and babble copies of the training list are `wav-reverberate` pipes inside wav.scp entries).  plan: one line per output utterance,
`out_key src_key [speed=F] [rir=ID] [noise=ID:snr:start_seconds[:bg]] ...` (misc/augment.py; speed=F resamples the source F * fs -> fs
before anything else meets it).  wav.scp: the sources, `key rxfilename` lines, the
rxfilename a RIFF PCM-16 file or a `command |` that writes one; rir.scp / noise.scp: the same for the impulse responses and noises the plan
names.  Every file must have --sample-frequency: without --resample-signals true there is no resampling; with it the impulse responses
and noises at another rate are resampled on the device when the pools are built (the `sox -r 8k` stages of egs/sre/v1/local/make_musan.sh;
the sources still must have --sample-frequency).  Writes out_dir/wav/<out_key>.wav (mono RIFF PCM-16) and
out_dir/wav.scp, and logs per key its samples, impulse response, number of noises and clipped samples.  The arithmetic is
wav-reverberate's with --normalize-output=true as include/xvector_hip.h restates it; --duration, --multi-channel-output and
--input-wave-channel are refused by name (misc/augment.py says why).
--make-plan writes one of the recipe's four lists to `plan` instead; the durations it needs are read from the files.  Its random choices
are this project's own (numpy.random.RandomState(--seed)), not those of Kaldi's reverberate_data_dir.py / augment_data_dir.py.
--make-speed-plan F[,F...] writes the speed-perturbed copies, `sp<F>-<key> <key> speed=<F>` per line and factor; no file is read.
"""
import sys
import time

import _cli
from misc import augment, waves

# utterances augmented together (Augmenter cuts them into calls that fit its workspace)
WINDOW_UTTERANCES = 256
WINDOW_SAMPLES = 64 << 20


def main():
    log = _cli.logger()
    args = _cli.parser_for("gpu", "aug_config", "sample_frequency", "rir_scp", "noise_scp", "resample_signals", "make_plan", "make_speed_plan", "seed",
                           "fg_interval", "plan", "wav_scp", "augment_out_dir").parse_args()
    fs = args.sample_frequency
    any_rate = args.resample_signals == "true"
    try:
        options = augment.AugmentOptions.from_conf(args.config) if args.config else augment.AugmentOptions()
        wavs = augment.read_scp(args.wav_scp)
        if args.make_speed_plan:
            entries = augment.make_speed_plan([key for key, _ in wavs], [f for f in args.make_speed_plan.split(",") if f], fs)
            augment.write_plan(entries, args.plan, fs)
            log.info("[INFO] Wrote the speed plan of %d utterances to %s." % (len(entries), args.plan))
            return
        rirs, noises, _ = augment.read_setup(options, args.rir_scp, args.noise_scp, fs, any_rate)
    except ValueError as e:
        sys.exit(str(e))
    mono = waves.WavFormat(fs)
    if args.make_plan:
        try:
            utterances = [(key, len(waves.read_wav(rx, mono, key)) / fs) for key, rx in wavs]
            entries = augment.make_plan(args.make_plan, utterances, augment.signal_seconds(rirs, fs), augment.signal_seconds(noises, fs),
                                        args.seed, args.fg_interval, fs)
        except ValueError as e:
            sys.exit(str(e))
        augment.write_plan(entries, args.plan, fs)
        log.info("[INFO] Wrote the %s plan of %d utterances to %s (seed %d)." % (args.make_plan, len(entries), args.plan, args.seed))
        return
    if not args.out_dir:
        sys.exit("out_dir is needed (unless --make-plan writes the plan)")
    rx_of = dict(wavs)
    try:
        entries = augment.read_plan(args.plan, fs, rirs, noises)
        augment.check_sources(entries, rx_of, args.plan, args.wav_scp)      # every key, before the device is opened
    except ValueError as e:
        sys.exit(str(e))
    device = _cli.device(args.gpu)
    aug = augment.Augmenter(options, rirs, noises, fs, device)
    out = waves.WavDir(args.out_dir)
    stats = {"utts": 0, "samples": 0, "clipped": 0, "t0": time.time()}
    window, window_samples = [], 0
    with open(out.scp_path, "w") as scp:
        def flush():
            if not window:
                return
            outs, clipped = aug.augment([w for _, w in window], [e for e, _ in window])
            for (e, _), y, c in zip(window, outs, clipped):
                scp.write(out.write(e.out_key, y, fs))
                log.info("[INFO] Key %s: %d samples, %srir %s, %d noises, %d clipped." % (e.out_key, len(y), "speed %s, " % e.speed if e.speed else "",
                                                                                         e.rir if e.rir is not None else "-", len(e.noises), int(c)))
                stats["utts"] += 1
                stats["samples"] += len(y)
                stats["clipped"] += int(c)
            del window[:]

        try:
            for e, samples in augment.plan_sources(entries, rx_of, mono, args.plan, args.wav_scp):
                window.append((e, samples))
                window_samples += len(samples)
                if len(window) >= WINDOW_UTTERANCES or window_samples >= WINDOW_SAMPLES:
                    flush()
                    window_samples = 0
        except augment.SourceError as err:
            sys.exit(str(err))
        flush()
    log.info("[INFO] Augmented %d utterances (%d samples, %d clipped) in %.2f s." % (stats["utts"], stats["samples"], stats["clipped"],
                                                                                    time.time() - stats["t0"]))


if __name__ == "__main__":
    main()
