#!/usr/bin/env python3
"""The training features of the recipe from the raw ones, on the GPU:

    python nnet/lib/prepare_feats.py [-g GPU] [--cmn-window 300] --vad scp:vad.scp [--cm-header {uniform,quartiles}]
                                     [--min-len N] [--write-utt2num-frames FILE] ark:raw_feats.ark ark,scp:out.ark,out.scp

Stage 4 of the recipe, for which the reference goes to Kaldi (egs/voxceleb/v1/run.sh:132-138, local/nnet3/xvector/prepare_feats_for_egs.sh:
apply-cmvn-sliding --norm-vars=false --center=true --cmn-window=300 | select-voiced-frames | copy-feats --compress=true
--write-num-frames): it writes the archive the loaders train from.  The raw archive (what make_mfcc.py wrote) is read as extract.py reads
its input; 'CM ' matrices go to the device undecoded, 'FM ' ones are uploaded; decode -> CMN -> selection -> 'CM ' encode run there
(misc/features.py FeaturePreparer: xv_cm_decode_ragged, xv_frontend, xv_cm_encode) and only the encoded bytes come back.
As select-voiced-frames does, an utterance with no voiced frame or with no entry in the VAD table is logged by key and skipped; a VAD
vector whose length differs from the frame count is an error that names the key.  --min-len N drops utterances of N frames or fewer
(counted after the selection) before they are encoded: the recipe's `$2 > min_len`.  --cm-header: where the header points of a column
lie - uniform (the default, as make_mfcc.py writes and for its reason) or quartiles (what copy-feats would choose).  --vad "" keeps every
frame.  Options of apply-cmvn-sliding that are not implemented (--norm-vars=true, --center=false) are not options of this program.
"""
import sys
import time

import numpy as np

import _cli
from misc import features
from misc.utils import prefetch_iter
from dataset.kaldi_io import VecFltTable, read_mat_ark_packed

# utterances gathered before they go to the GPU together (FeaturePreparer cuts them into calls that fit its workspace)
WINDOW_UTTERANCES = 512
WINDOW_FRAMES = 400000


def main():
    log = _cli.logger(batched=True)
    args = _cli.parser_for("gpu", "prep_cmn_window", "vad", "cm_header", "min_len", "write_utt2num_frames", "raw_rspecifier",
                           "prepared_wspecifier").parse_args()
    if args.cmn_window < 0:
        sys.exit("--cmn-window must be 0 (off) or a number of frames")
    if "." in args.raw_rspecifier and args.raw_rspecifier.rsplit(".", 1)[1] == "scp":
        sys.exit("The rspecifier must be ark or input pipe")
    out = _cli.Table(args.prepared_wspecifier, "prepared_wspecifier")
    device = _cli.device(args.gpu)
    prep = features.FeaturePreparer(args.cmn_window, args.cm_header, device)
    vad = VecFltTable(args.vad) if args.vad else None
    counts = open(args.write_utt2num_frames, "w") if args.write_utt2num_frames else None
    stats = {"utts": 0, "frames": 0, "skipped": 0, "short": 0, "t0": time.time()}
    window = []

    def flush():
        images = prep.prepare([f for _, f, _, _ in window], [m for _, _, m, _ in window])
        for (key, _, _, frames), image in zip(window, images):
            out.write(key, lambda fd, k: features.write_cm_image(fd, image, key=k))
            if counts is not None:
                counts.write("%s %d\n" % (key, frames))
            stats["utts"] += 1
            stats["frames"] += frames
        del window[:]
        for h in log.root.handlers:
            h.flush()

    window_frames = 0
    for key, feature in prefetch_iter(read_mat_ark_packed(args.raw_rspecifier), depth=2 * WINDOW_UTTERANCES):
        frames, mask = int(feature.shape[0]), None
        if vad is not None:
            decisions = vad.get(key)
            if decisions is None:
                log.info("[INFO] Key %s has no VAD entry, skip." % key)
                stats["skipped"] += 1
                continue
            if len(decisions) != frames:
                sys.exit("Key %s: %d frames but %d VAD decisions" % (key, frames, len(decisions)))
            mask = np.ascontiguousarray(np.asarray(decisions) != 0).view(np.uint8)
            frames = int(np.count_nonzero(mask))
        if frames == 0:
            log.info("[INFO] Key %s has no voiced frame, skip." % key)
            stats["skipped"] += 1
            continue
        if frames <= args.min_len:
            log.info("[INFO] Key %s length too short, %d <= %d, skip." % (key, frames, args.min_len))
            stats["short"] += 1
            continue
        if getattr(feature, "dtype", np.float32) != np.float32:
            feature = np.asarray(feature, np.float32)
        window.append((key, feature, mask, frames))
        window_frames += int(feature.shape[0])
        if len(window) >= WINDOW_UTTERANCES or window_frames >= WINDOW_FRAMES:
            flush()
            window_frames = 0
    if window:
        flush()
    out.close()
    if counts is not None:
        counts.close()
    if vad is not None:
        vad.close()
    log.info("[INFO] Prepared %d utterances (%d frames) in %.2f s, skipped %d without voiced frames or VAD entry and %d of %d frames or fewer."
             % (stats["utts"], stats["frames"], time.time() - stats["t0"], stats["skipped"], stats["short"], args.min_len))


if __name__ == "__main__":
    main()
