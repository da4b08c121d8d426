#!/usr/bin/env python3
"""Drop-in for egs/voxceleb/v1/nnet/lib/extract.py (same CLI, wrap/extract_wrapper.sh:39-40):

    python nnet/lib/extract.py [-g GPU] [-m MIN] [-s CHUNK] [-n] [--node NAME] [--cmn-window N] [--vad RSPECIFIER] model_dir rspecifier wspecifier
    python nnet/lib/extract.py [...] --mfcc-config CONF | --fbank-config CONF [--vad-config CONF] [--cmn-window N] model_dir wav.scp wspecifier

Reads an ark / input pipe of feature matrices, writes a Kaldi float-vector ark of embeddings
(is_training=False graph, moving BN statistics).  Utterances longer than --chunk-size are cut into
half-overlapping chunks whose embeddings are length-weighted averaged (reference extract.py:65-94).
-g selects the HIP device (the reference's CPU mode `-g -1` maps to device 0: there is no CPU path).
--cmn-window / --vad (not in the reference's CLI) take over the two Kaldi programs the recipe pipes in front of this script
(run_extract_embeddings.sh:47: apply-cmvn-sliding --cmn-window=300 | select-voiced-frames): the rspecifier then names the RAW features,
both steps run on the GPU behind the 'CM ' decode (Trainer.predict_batch: model/predict.py), and every length - --min-chunk-size, --chunk-size, the log
lines - counts the frames left after selection, as it does behind the pipe.
--mfcc-config / --fbank-config (exactly one): the rspecifier names a wav.scp, read as make_mfcc.py reads it (paths and `cmd |` entries, its
rate rules, its error texts), and the whole chain runs on the device: PCM upload -> (resample) -> xv_mfcc / xv_fbank -> xv_energy_vad
(--vad-config; without it every frame is kept) -> xv_frontend (--cmn-window, selection) -> forward.  Between the upload and the read-back
of the embeddings only per-utterance counts come to the host (frames kept; samples clipped by a resampling): no feature archive, no
vad.scp, no 'CM ' rounding in between.  Log lines, skip lines, output order, chunk averaging and the rate line are those of
make_mfcc.py --compress false followed by this program with --cmn-window N --vad scp:; an utterance too short for a frame gets
make_mfcc.py's skip line.  Refused: both config options, --vad beside them (--vad-config computes the decisions), an ark: rspecifier
with them, features whose dimension is not nnet/feature_dim.
"""
import logging
import os
import sys
import time

import _cli
from model.trainer import Trainer
from misc.utils import Params, EmbeddingWindow, prefetch_iter, select_voiced
from dataset.kaldi_io import open_or_fd, read_mat_ark_packed, write_vec_flt, DeviceRows, VecFltTable, VoicedRows

# utterances gathered before they go to the GPU together (sorted by length into padded batches: Trainer.predict_batch, model/predict.py); results are
# written in archive order.  One utterance per forward, as the reference runs (extract.py:64-93), left the chip at 9-20 % of its
# training-pass rate at real utterance lengths (profiles/r03_extract_bench.txt).
WINDOW_UTTERANCES = 512
WINDOW_FRAMES = 400000


def main():
    log = _cli.logger(batched=True)
    args = _cli.parser_for("gpu", "min_chunk_size", "chunk_size", "normalize", "node", "cmn_window", "vad", "wav_mfcc_config", "wav_fbank_config",
                           "wav_vad_config", "model_dir", "rspecifier", "wspecifier").parse_args()
    wav_mode = bool(args.mfcc_config or args.fbank_config)      # the rspecifier names a wav.scp; the features are computed here
    if args.mfcc_config and args.fbank_config:
        sys.exit("--mfcc-config and --fbank-config: exactly one of them names the features")
    if args.vad_config and args.vad:
        sys.exit("--vad and --vad-config: --vad reads the decisions of an archive of features, --vad-config computes them from the waveforms "
                 "(with --mfcc-config or --fbank-config); give one")
    if args.vad_config and not wav_mode:
        sys.exit("--vad-config computes the decisions from waveforms: it needs --mfcc-config or --fbank-config (the VAD of a feature archive comes with --vad)")
    if wav_mode and args.vad:
        sys.exit("--vad reads the decisions of an archive of features; with --mfcc-config / --fbank-config they are computed here (--vad-config)")
    if wav_mode and args.rspecifier.startswith("ark:"):
        sys.exit("--mfcc-config / --fbank-config: the rspecifier names a wav.scp, not an archive of features (got %s)" % args.rspecifier)
    if wav_mode:
        from misc import features
        try:
            options = features.MfccOptions.from_conf(args.mfcc_config) if args.mfcc_config else features.FbankOptions.from_conf(args.fbank_config)
            vad_options = features.VadOptions.from_conf(args.vad_config) if args.vad_config else None
        except ValueError as e:
            sys.exit(str(e))
    # -g is an enable flag in the reference ("an arbitrary number except -1"; run_extract_embeddings.sh passes the JOB
    # number with --gpuid), device choice being left to CUDA_VISIBLE_DEVICES.  Here: among the devices HIP_VISIBLE_DEVICES
    # leaves visible, job N takes device N modulo their count, so `nj` parallel jobs spread over the GPUs of the node and
    # a node with one device serves every job; -1 (the default) = the first visible device.
    if args.gpu >= 0:
        os.environ["LOCAL_RANK"] = str(_cli.device_index(args.gpu))
    nnet_dir = os.path.join(args.model_dir, "nnet")
    config_json = os.path.join(args.model_dir, "nnet/config.json")
    if not os.path.isfile(config_json):
        sys.exit("Cannot find params.json in %s" % config_json)
    params = Params(config_json)
    if len(args.node) != 0:
        params.embedding_node = args.node
    log.info("Extract embedding from %s" % params.embedding_node)
    trainer = Trainer(params, args.model_dir, single_cpu=True)
    with open(os.path.join(nnet_dir, "feature_dim"), "r") as f:
        dim = int(f.readline().strip())
    if wav_mode and options.feature_dim() != dim:
        sys.exit("%s gives features of %d dimensions, but the model's nnet/feature_dim is %d"
                 % ("--mfcc-config" if args.mfcc_config else "--fbank-config", options.feature_dim(), dim))
    trainer.build("predict", dim=dim)
    if not wav_mode and "." in args.rspecifier and args.rspecifier.rsplit(".", 1)[1] == "scp":
        sys.exit("The rspecifier must be ark or input pipe")
    if args.cmn_window < 0:
        sys.exit("--cmn-window must be 0 (off) or a number of frames")
    vad = VecFltTable(args.vad) if len(args.vad) != 0 else None
    fp_out = open_or_fd(args.wspecifier, "wb")
    window, window_frames = [], 0
    pending = []           # the window whose forward passes are on the GPU while the next one is read, planned and enqueued
    stats = {"utts": 0, "frames": 0, "t0": time.time(), "warm": None}      # warm: (time, utterances, frames) once the first window is done

    def submit():
        entries = list(window)
        del window[:]
        keep = [feature for _, feature, skip in entries if skip is None and feature.shape[0] >= args.min_chunk_size]
        job = EmbeddingWindow(lambda pieces: trainer.predict_batch(pieces, return_device=True, cmn_window=args.cmn_window), keep, args.chunk_size,
                              args.normalize)
        finish()           # the previous window: read back, log, write - while this one runs
        pending.append((entries, job))

    def finish():
        if not pending:
            return
        entries, job = pending.pop()
        results = iter(job.results())
        for key, feature, skip in entries:   # log lines and output vectors in archive order, as the one-at-a-time loop gives them
            if skip is not None:             # dropped by the voiced-frame selection (no VAD entry, wrong length, nothing voiced)
                log.info(skip)
                continue
            frames = feature.shape[0]
            if frames < args.min_chunk_size:
                log.info("[INFO] Key %s length too short, %d < %d, skip." % (key, frames, args.min_chunk_size))
                continue
            embedding, pieces = next(results)
            log.info("[INFO] Key %s length %d%s." % (key, frames, "" if pieces == 1 else " > %d, split to %d segments" % (args.chunk_size, pieces)))
            write_vec_flt(fp_out, embedding, key=key)
            stats["utts"] += 1
            stats["frames"] += frames
        if stats["warm"] is None:
            stats["warm"] = (time.time(), stats["utts"], stats["frames"])
        for h in logging.getLogger().handlers:
            h.flush()

    def archive_entries():
        """(key, feature, skip line or None, True) per matrix of the archive.  The reader runs ahead of the GPU in its own thread; 'CM '
        matrices arrive undecoded (kaldi_io.PackedMatrix) and are decoded on the GPU."""
        for key, feature in prefetch_iter(read_mat_ark_packed(args.rspecifier), depth=2 * WINDOW_UTTERANCES):
            skip = None
            if vad is not None:              # from here on `feature` counts voiced frames: the raw matrix, its mask, nothing selected yet
                feature, skip = select_voiced(key, feature, vad.get(key))
            elif args.cmn_window > 0:
                feature = VoicedRows(feature)
            yield key, feature, skip, True

    def wav_entries(fx):
        """wav mode: the same per entry of the wav.scp.  The files read so far go to the device together (FeatureExtractor.device_batches)
        once they are WINDOW_UTTERANCES or hold WINDOW_FRAMES raw frames; an utterance becomes a DeviceRows - its features and its mask stay
        on the device - or a skip line.  The last field is False for an utterance too short for one frame: make_mfcc.py would not have
        written it, so it does not count towards a window - the windows, and with them the padded batches and the bits of the embeddings,
        are those of the two-step path."""
        wavs, frames = [], 0

        def entries():
            got = {}
            for members, samples, batch in fx.device_batches([w for _, w, _ in wavs], [rate for _, _, rate in wavs]):
                for j, (i, n) in enumerate(zip(members, samples)):
                    key, _, rate = wavs[i]
                    if rate != options.sample_frequency:
                        log.info("[INFO] Key %s: resampled from %d Hz." % (key, rate))
                    if batch is None or batch.frames[j] == 0:
                        got[i] = (key, None, "[INFO] Key %s has %d samples, too few for one frame, skip." % (key, n), False)
                    elif batch.kept[j] == 0:
                        got[i] = (key, None, "[INFO] Key %s has no voiced frame, skip." % key, True)
                    else:
                        got[i] = (key, DeviceRows(batch, j), None, True)
            del wavs[:]
            return [got[i] for i in range(len(got))]

        for key, wav, rate in prefetch_iter(features.read_wav_scp(args.rspecifier, options), depth=2 * WINDOW_UTTERANCES):
            wavs.append((key, wav, rate))
            frames += fx.num_frames(int(len(wav) * options.sample_frequency / max(rate, 1)))
            if len(wavs) >= WINDOW_UTTERANCES or frames >= WINDOW_FRAMES:
                frames = 0
                for entry in entries():
                    yield entry
        if wavs:
            for entry in entries():
                yield entry

    source = archive_entries() if not wav_mode else \
        wav_entries(features.FeatureExtractor(options, vad_options, str(trainer.engine.device), with_vad=vad_options is not None))
    window_utts = 0
    try:
        for key, feature, skip, counted in source:
            window.append((key, feature, skip))
            window_utts += counted
            window_frames += feature.shape[0] if skip is None else 0
            if window_utts >= WINDOW_UTTERANCES or window_frames >= WINDOW_FRAMES:
                submit()
                window_utts = window_frames = 0
    except ValueError as e:
        if not wav_mode:
            raise
        sys.exit(str(e))       # the reader's refusals (a malformed line, a file at another rate, ...), as make_mfcc.py words them
    submit()
    finish()
    now = time.time()
    t1, u1, f1 = stats["warm"] or (now, 0, 0)
    rate = ", %.0f utterances/s = %.2f M frames/s after the first window" % ((stats["utts"] - u1) / (now - t1), (stats["frames"] - f1) / (now - t1) / 1e6) \
        if stats["utts"] > u1 and now > t1 else ""
    log.info("[INFO] Extracted %d utterances (%d frames) in %.2f s%s." % (stats["utts"], stats["frames"], now - stats["t0"], rate))
    fp_out.close()
    if vad is not None:
        vad.close()
    trainer.close()


if __name__ == "__main__":
    main()
