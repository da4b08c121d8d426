#!/usr/bin/env python3
"""MFCC features and energy VAD decisions from a wav.scp on the GPU:

    python nnet/lib/make_mfcc.py [-g GPU] [--mfcc-config conf/mfcc.conf] [--vad-config conf/vad.conf] [--compress {true,false}]
                                 [--write-utt2num-frames FILE]
                                 [--augment-plan PLAN --rir-scp F --noise-scp F [--augment-config conf] [--resample-signals true]]
                                 wav.scp ark,scp:feats.ark,feats.scp ark,scp:vad.ark,vad.scp

The first stage of the recipe, for which the reference goes to Kaldi (egs/voxceleb/v1/run.sh:59-63: steps/make_mfcc.sh --mfcc-config
conf/mfcc.conf = compute-mfcc-feats | copy-feats --compress=true, then sid/compute_vad_decision.sh = compute-vad-decision).  wav.scp:
`key rxfilename` lines, the rxfilename a RIFF PCM-16 file or a `command |` that writes one.  The feature archive ('CM ' matrices with
--compress=true, the default; 'FM ' otherwise) and the archive of VAD decisions (float vectors of 1 / 0 per frame) are what
extract.py --cmn-window 300 --vad scp:vad.scp and the loaders read.  `ark:FILE` alone writes no scp.  The 'CM ' matrices carry evenly spaced
header points per column, not copy-feats' quartiles: the same format for every reader, and a rounding error below (max - min) / 255 of
the column whatever its distribution (dataset/kaldi_io.py write_compressed_mat, header="uniform"; the compression itself runs on the
device, xv_cm_encode, which gives that function's bytes, so one byte per value comes back to the host instead of four).
This is the --dither=0 program: the conf may say --dither=0, any other value is refused (misc/features.py says why); so is every other
option of the two Kaldi programs that is not implemented, by name.  An utterance too short for one frame is logged and skipped.
--augment-plan: the features of the AUGMENTED training list (egs/voxceleb/v1/run.sh:68-130) without a wav file in between - the keys
written are the plan's output keys (misc/augment.py: `out_key src_key [rir=ID] [noise=ID:snr:start_seconds[:bg]] ...`), the sources come
from wav.scp, and the reverberated / noisy PCM goes from the augmentation kernels to the MFCC kernels on the device: the same bytes as
nnet/lib/augment.py followed by this program on its wav.scp.  Without the option nothing changes.
--allow-downsample=true / --allow-upsample=true in the MFCC conf (compute-mfcc-feats' options): files at a higher / lower rate than
--sample-frequency are read at their own rate and resampled on the device in front of the MFCC kernels, grouped by rate (misc/resample.py:
the same bytes as nnet/lib/resample.py --to-rate followed by this program on its wav.scp; the samples are rounded to int16 in between, where
compute-mfcc-feats keeps floats).  Without them a file at another rate is refused, as before.
make_fbank.py is this program with --fbank-config (main("fbank")); extract.py --mfcc-config / --fbank-config reads the same wav.scp with
the same reader and goes on to the embeddings without writing either table.
"""
import sys
import time

import numpy as np

import _cli
from misc import augment, features
from dataset import kaldi_io

# utterances read before they go to the GPU together (FeatureExtractor cuts them into calls that fit its workspace)
WINDOW_UTTERANCES = 256
WINDOW_SAMPLES = 64 << 20


def main(kind="mfcc"):
    """kind "mfcc": this program.  "fbank": make_fbank.py - --fbank-config in place of --mfcc-config (misc.features.FbankOptions), the VAD
    wspecifier optional; everything else, `mfcc` the feature options of either kind, is the code below."""
    log = _cli.logger()
    args = _cli.parser_for("gpu", kind + "_config", "vad_config", "compress", "write_utt2num_frames", "augment_plan", "rir_scp", "noise_scp",
                           "augment_config", "resample_signals", "wav_scp", "feats_wspecifier",
                           "vad_wspecifier" if kind == "mfcc" else "vad_wspecifier_optional").parse_args()
    options_of, conf = (features.FbankOptions if kind == "fbank" else features.MfccOptions), getattr(args, kind + "_config")
    try:
        mfcc = options_of.from_conf(conf) if conf else options_of()
        vad = features.VadOptions.from_conf(args.vad_config) if args.vad_config else features.VadOptions()
    except ValueError as e:
        sys.exit(str(e))
    device = _cli.device(args.gpu)
    log.info("[INFO] %s without dither (--dither=0): on digital silence the features sit at the FLT_EPSILON floors; --energy-floor lifts the energy."
             % ("MFCC" if kind == "mfcc" else "Filterbank energies"))
    fx = features.FeatureExtractor(mfcc, vad, device, with_vad=bool(args.vad_wspecifier))
    feats_out = _cli.Table(args.feats_wspecifier, "feats_wspecifier")
    vad_out = _cli.Table(args.vad_wspecifier, "vad_wspecifier") if args.vad_wspecifier else None      # make_fbank.py may leave it out
    counts = open(args.write_utt2num_frames, "w") if args.write_utt2num_frames else None
    # 'CM ' with evenly spaced header points: the rounding error stays below (max - min) / 255 of a column whatever its distribution
    # (Kaldi's quartile points let it reach (max - min) / 126); every 'CM ' reader decodes it.  The matrices are compressed on the device
    # (ops.cm_encode: the bytes kaldi_io.write_compressed_mat(header="uniform") gives) and come back as the images the archive holds
    cm_header = "uniform" if args.compress == "true" else None
    write_mat = features.write_cm_image if cm_header else kaldi_io.write_mat
    stats = {"utts": 0, "frames": 0, "voiced": 0, "skipped": 0, "t0": time.time()}
    window, rates, window_samples = [], [], 0

    def write(key, samples, feats, decisions):
        frames = len(decisions) if decisions is not None else features.rows_of(feats, fx.dim)
        if frames == 0:
            log.info("[INFO] Key %s has %d samples, too few for one frame, skip." % (key, samples))
            stats["skipped"] += 1
            return
        voiced = int(decisions.sum()) if decisions is not None else 0
        log.info("[INFO] Key %s: %d samples, %d frames%s." % (key, samples, frames, ", %d voiced" % voiced if decisions is not None else ""))
        feats_out.write(key, lambda fd, k: write_mat(fd, feats, key=k))
        if vad_out is not None:
            vad_out.write(key, lambda fd, k: kaldi_io.write_vec_flt(fd, decisions, key=k))
        if counts is not None:
            counts.write("%s %d\n" % (key, frames))
        stats["utts"] += 1
        stats["frames"] += frames
        stats["voiced"] += voiced

    def flush():
        if all(rate == mfcc.sample_frequency for rate in rates):
            results = fx.extract([w for _, w in window], cm_header)
        else:
            results = fx.extract_at_rates([w for _, w in window], rates, cm_header)
        for (key, w), rate, (feats, decisions) in zip(window, rates, results):
            if rate != mfcc.sample_frequency:
                log.info("[INFO] Key %s: resampled from %d Hz." % (key, rate))
            write(key, len(w), feats, decisions)
        del window[:]
        del rates[:]

    def flush_augmented(aug):
        pcm, offsets, lengths, clipped = aug.run([w for _, w in window], [e for e, _ in window])
        results = fx.extract_packed(pcm, offsets, lengths, cm_header)
        for (e, _), n, c, (feats, decisions) in zip(window, lengths, clipped, results):
            log.info("[INFO] Key %s: augmented from %s, rir %s, %d noises, %d clipped." % (e.out_key, e.src_key, e.rir if e.rir is not None else "-",
                                                                                          len(e.noises), int(c)))
            write(e.out_key, int(n), feats, decisions)
        del window[:]

    any_rate = args.resample_signals == "true"
    if not args.augment_plan and (args.rir_scp or args.noise_scp or args.augment_config or any_rate):
        sys.exit("--rir-scp, --noise-scp, --augment-config and --resample-signals belong to --augment-plan")
    if args.augment_plan:
        try:
            options = augment.AugmentOptions.from_conf(args.augment_config) if args.augment_config else augment.AugmentOptions()
            fs = mfcc.sample_frequency
            rirs, noises, entries = augment.read_setup(options, args.rir_scp, args.noise_scp, fs, any_rate, args.augment_plan)
            rx_of = dict(augment.read_scp(args.wav_scp))
        except ValueError as e:
            sys.exit(str(e))
        aug = augment.Augmenter(options, rirs, noises, fs, device)
        try:
            for e, samples in augment.plan_sources(entries, rx_of, mfcc, args.augment_plan, args.wav_scp):
                window.append((e, samples))
                window_samples += len(samples)
                if len(window) >= WINDOW_UTTERANCES or window_samples >= WINDOW_SAMPLES:
                    flush_augmented(aug)
                    window_samples = 0
        except augment.SourceError as err:
            sys.exit(str(err))
        if window:
            flush_augmented(aug)
    else:
        try:
            for key, wav, rate in features.read_wav_scp(args.wav_scp, mfcc):
                window.append((key, wav))
                rates.append(rate)
                window_samples += len(wav)
                if len(window) >= WINDOW_UTTERANCES or window_samples >= WINDOW_SAMPLES:
                    flush()
                    window_samples = 0
        except ValueError as e:
            sys.exit(str(e))
        flush()
    feats_out.close()
    if vad_out is not None:
        vad_out.close()
    if counts is not None:
        counts.close()
    log.info("[INFO] Computed features of %d utterances (%d frames%s) in %.2f s, skipped %d."
             % (stats["utts"], stats["frames"], ", %d voiced" % stats["voiced"] if vad_out is not None else "", time.time() - stats["t0"], stats["skipped"]))


if __name__ == "__main__":
    main()
