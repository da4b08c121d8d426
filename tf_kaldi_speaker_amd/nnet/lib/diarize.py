#!/usr/bin/env python3
"""Speaker diarization with the x-vector network: what Kaldi's callhome_diarization/v2 recipe does between the features and the RTTM
(extract_xvectors.sh's sliding windows, score_plda.sh, cluster.sh, make_rttm.py), restated - nothing is compared with a Kaldi run:

    python nnet/lib/diarize.py [-g GPU] [--cmn-window 300] [--window 1.5 --period 0.75 --min-segment 0.5] [--segments FILE | --vad RSPECIFIER]
                               [--backend DIR --scoring {cosine,lda_cos,plda} [--target-energy F]] (--threshold T | --reco2num-spk FILE)
                               [--vbx [--vbx-fa 0.3 --vbx-fb 17 --vbx-loop-prob 0.99 --vbx-max-iters 20 --vbx-epsilon 1e-4 --vbx-init-smoothing 5]]
                               [--first-pass-max-points 2048] [--write-embeddings WSPECIFIER] model_dir rspecifier rttm_out

rspecifier: an ark (or input pipe) of RAW feature matrices, one per recording, at a frame shift of 10 ms.  Per recording: sliding-window
CMN over the whole recording on the GPU (ops.frontend; as in the recipe it runs before the cut and no frame is removed); the speech
segments (--segments: a Kaldi segments file; --vad: the voiced runs of the decisions; neither: the whole recording) are cut into windows
(misc/diarization.py subsegments); the windows - row ranges of the normalised recording, gathered on the device - go through
Trainer.predict_batch as device rows.  Then misc/diarization.py Diarizer: all-pairs scores per recording (cosine, or behind --backend the
LDA cosine or the PLDA log-likelihood ratio - with --target-energy F behind ivector-plda-scoring-dense's per-recording PCA: each recording
scored with the PLDA model projected into the leading directions of its own windows that hold F of the energy (xv_backend_pca_plda:
DESIGN.md section 6k; one log line per recording gives the kept dimension; off by default, and then every output is what it was without
the option), agglomerative clustering on the GPU (xv_ahc_cluster) down to --threshold or to the
recording's entry in --reco2num-spk - a recording of more than --first-pass-max-points windows (Kaldi's option and default, 2048) in two
passes, as agglomerative-cluster does it: contiguous subsets down to ten times the wanted clusters, then the survivors against each other
over the whole score matrix (xv_ahc_cluster_from, xv_ahc_cluster_sums: DESIGN.md section 6l; up to 32768 windows); with --vbx the clusterer's labels (it should stop early: too many speakers) start the VB-HMM
clustering of the windows in the PLDA space (VBx, xv_vbx: DESIGN.md section 6j), which re-assigns them and drops redundant speakers - one log
line per recording says speakers before and after, iterations and the last ELBO; and the turns: overlapping windows are cut at the midpoint
of the overlap, abutting windows of one speaker merged.  Output: `SPEAKER <recording> 0 <start> <duration> <NA> <NA> <speaker> <NA> <NA>` lines, speakers numbered from 1 per
recording.  --write-embeddings: the windows' embeddings, keyed `recording-startframe-endframe`.
Refused: both or neither of --threshold / --reco2num-spk, --segments beside --vad, a back end without a --scoring that uses it (and the
reverse), --vbx without --scoring plda or with an option outside its range, --target-energy without --scoring plda or outside (0, 1], a --min-segment below the network's receptive field, a --first-pass-max-points outside 2 .. 2048, a recording of more than 32768 windows, a
recording of more than 2048 windows together with --vbx or --target-energy (their kernels keep the cap of 2048), a recording whose first pass
leaves more than 2048 clusters, a recording without an entry in --reco2num-spk.
Not here: waveform input (make_mfcc.py writes the archive this reads), overlap detection; tune_diarization.py chooses
the --threshold on a development set.
"""
import os
import sys

import numpy as np

import _cli
import _lib      # (the caps of the kernels: no device library loads)
from misc import diarization

FRAME_SHIFT = 0.01      # seconds per frame of the features


def window_key(reco, start, end):
    return "%s-%07d-%07d" % (reco, start, end)


def read_reco2num_spk(path):
    out = {}
    with open(path, "r") as f:
        for no, line in enumerate(f, 1):
            cols = line.split()
            if not cols:
                continue
            if len(cols) != 2 or not cols[1].isdigit() or int(cols[1]) < 1:
                raise ValueError("%s:%d: `recording speakers` with a positive count is expected" % (path, no))
            out[cols[0]] = int(cols[1])
    return out


def window_embeddings(trainer, ops, torch, matrix, windows, cmn_window):
    """Embeddings float32 [len(windows), E] of the frame ranges `windows` of one recording (host float32 [T, d]): CMN once over the whole
    recording on the device, the windows gathered there into one padded block that predict_batch takes as device rows."""
    from dataset.kaldi_io import DeviceBatch, DeviceRows
    dev = trainer.engine.device
    frames = matrix.shape[0]
    x = torch.from_numpy(np.ascontiguousarray(matrix[None], dtype=np.float32)).to(dev)
    y, _ = ops.frontend(x, torch.tensor([frames], dtype=torch.int32, device=dev), cmn_window)
    starts = np.asarray([s for s, _ in windows], np.int64)
    lengths = np.asarray([e - s for s, e in windows], np.int64)
    index = np.minimum(starts[:, None] + np.arange(int(lengths.max()))[None, :], frames - 1)      # (rows beyond a window's length are padding)
    block = y[0][torch.from_numpy(index).to(dev)]
    batch = DeviceBatch(block, torch.from_numpy(lengths.astype(np.int32)).to(dev), None, lengths, lengths)
    return trainer.predict_batch([DeviceRows(batch, k) for k in range(len(windows))])


def main():
    log = _cli.logger()
    args = _cli.parser_for("gpu", "prep_cmn_window", "window", "period", "min_segment", "segments", "diar_vad", "backend", "diar_scoring", "threshold",
                           "reco2num_spk", "vbx", "vbx_fa", "vbx_fb", "vbx_loop_prob", "vbx_max_iters", "vbx_epsilon", "vbx_init_smoothing", "target_energy", "first_pass_max_points", "write_embeddings", "model_dir", "rspecifier", "rttm_out").parse_args()
    if (args.threshold is None) == (not args.reco2num_spk):
        sys.exit("exactly one of --threshold and --reco2num-spk says when the merging stops")
    if args.segments and args.vad:
        sys.exit("--segments and --vad: both name the speech of a recording; give one")
    if args.scoring != "cosine" and not args.backend:
        sys.exit("--scoring %s needs --backend DIR (a directory written by train_backend.py)" % args.scoring)
    if args.backend and args.scoring == "cosine":
        sys.exit("--backend is given but --scoring is cosine: choose --scoring lda_cos or plda")
    if args.vbx and args.scoring != "plda":
        sys.exit("--vbx needs --scoring plda (VBx models the windows in the PLDA space of --backend), not --scoring %s" % args.scoring)
    if args.vbx and not (0.0 < args.vbx_loop_prob < 1.0 and args.vbx_fa > 0 and args.vbx_fb > 0 and 1 <= args.vbx_max_iters <= _lib.VBX_MAX_ITERS
                         and args.vbx_init_smoothing >= 0 and args.vbx_epsilon == args.vbx_epsilon):
        sys.exit("--vbx: --vbx-loop-prob must lie strictly between 0 and 1, --vbx-fa and --vbx-fb be positive, --vbx-max-iters lie in 1 .. %d, "
                 "--vbx-init-smoothing not be negative" % _lib.VBX_MAX_ITERS)
    if args.target_energy is not None and args.scoring != "plda":
        sys.exit("--target-energy needs --scoring plda (the per-recording PCA projects the PLDA model of --backend), not --scoring %s" % args.scoring)
    if args.target_energy is not None and not 0.0 < args.target_energy <= 1.0:
        sys.exit("--target-energy must lie in (0, 1] (got %g)" % args.target_energy)
    if not 2 <= args.first_pass_max_points <= diarization.FIRST_PASS_CAP:
        sys.exit("--first-pass-max-points must lie in 2 .. %d (got %d)" % (diarization.FIRST_PASS_CAP, args.first_pass_max_points))
    if args.cmn_window < 0:
        sys.exit("--cmn-window must be 0 (off) or a number of frames")
    window, period, min_segment = (int(round(v / FRAME_SHIFT)) for v in (args.window, args.period, args.min_segment))
    if window <= 0 or period <= 0 or min_segment <= 0:
        sys.exit("--window, --period and --min-segment must be at least one frame (%g s)" % FRAME_SHIFT)
    if "." in args.rspecifier and args.rspecifier.rsplit(".", 1)[1] == "scp":
        sys.exit("The rspecifier must be ark or input pipe")
    try:
        reco2num_spk = read_reco2num_spk(args.reco2num_spk) if args.reco2num_spk else None
        segments = {}
        if args.segments:
            for _, reco, start, end in diarization.read_segments(args.segments):
                segments.setdefault(reco, []).append((int(round(start / FRAME_SHIFT)), int(round(end / FRAME_SHIFT))))
    except ValueError as e:
        sys.exit(str(e))
    # (the refusals above come before the imports that load the device libraries)
    from model.trainer import Trainer
    from misc.utils import Params
    from dataset.kaldi_io import PackedMatrix, VecFltTable, open_or_fd, read_mat_ark_packed, write_vec_flt
    if args.gpu >= 0:
        os.environ["LOCAL_RANK"] = str(_cli.device_index(args.gpu))
    nnet_dir = os.path.join(args.model_dir, "nnet")
    config_json = os.path.join(nnet_dir, "config.json")
    if not os.path.isfile(config_json):
        sys.exit("Cannot find params.json in %s" % config_json)
    params = Params(config_json)
    trainer = Trainer(params, args.model_dir, single_cpu=True)
    with open(os.path.join(nnet_dir, "feature_dim"), "r") as f:
        dim = int(f.readline().strip())
    trainer.build("predict", dim=dim)
    if min_segment < trainer.engine.min_frames:
        sys.exit("--min-segment %g s is %d frames, fewer than the network's receptive field (%d)" % (args.min_segment, min_segment, trainer.engine.min_frames))
    from _host import device_ops
    torch, ops, device = device_ops(str(trainer.engine.device))
    vad = VecFltTable(args.vad) if args.vad else None
    fp_emb = open_or_fd(args.write_embeddings, "wb") if args.write_embeddings else None
    embeddings, windows_of = {}, {}
    for reco, feature in read_mat_ark_packed(args.rspecifier):
        matrix = feature.decode() if isinstance(feature, PackedMatrix) else np.asarray(feature, np.float32)
        frames = matrix.shape[0]
        if matrix.shape[1] != dim:
            sys.exit("recording %s has features of %d dimensions, but the model's nnet/feature_dim is %d" % (reco, matrix.shape[1], dim))
        if reco in embeddings:
            sys.exit("recording %s appears twice in %s" % (reco, args.rspecifier))
        if args.segments:
            speech = [(min(s, frames), min(e, frames)) for s, e in segments.get(reco, [])]
        elif vad is not None:
            decisions = vad.get(reco)
            if decisions is not None and len(decisions) != frames:
                sys.exit("recording %s has %d frames, its VAD entry %d" % (reco, frames, len(decisions)))
            speech = [] if decisions is None else diarization.speech_segments(decisions)
        else:
            speech = [(0, frames)]
        windows = [w for s, e in speech for w in diarization.subsegments(s, e, window, period, min_segment, log)]
        if not windows:
            log.info("[INFO] Recording %s: no speech segment of %d frames or more, skip." % (reco, min_segment))
            continue
        emb = window_embeddings(trainer, ops, torch, matrix, windows, args.cmn_window)
        log.info("[INFO] Recording %s: %d frames, %d speech segments, %d windows." % (reco, frames, len(speech), len(windows)))
        if fp_emb is not None:
            for (s, e), vec in zip(windows, emb):
                write_vec_flt(fp_emb, vec, key=window_key(reco, s, e))
        embeddings[reco], windows_of[reco] = emb, windows
    if fp_emb is not None:
        fp_emb.close()
    if vad is not None:
        vad.close()
    if not embeddings:
        sys.exit("no recording with speech in %s" % args.rspecifier)
    try:
        if args.backend:
            from misc import backend as B
            be = B.Backend.load(args.backend)
            d_emb = next(iter(embeddings.values())).shape[1]
            if be.d != d_emb:
                sys.exit("dimension mismatch: the embeddings have %d dimensions, the back end %s works on %d" % (d_emb, args.backend, be.d))
            if args.scoring == "plda" and be.plda is None:
                sys.exit("--scoring plda: the back end %s holds no plda file" % args.backend)
            scorer = B.BackendScorer(be, args.scoring, str(device))
        else:
            from misc import scoring
            scorer = scoring.CosineScorer(str(device))
        vbx = None
        if args.vbx:
            vbx = diarization.VbxOptions(fa=args.vbx_fa, fb=args.vbx_fb, loop_prob=args.vbx_loop_prob, max_iters=args.vbx_max_iters,
                                         epsilon=args.vbx_epsilon, init_smoothing=args.vbx_init_smoothing)
        diarizer = diarization.Diarizer(scorer, threshold=args.threshold, reco2num_spk=reco2num_spk, vbx=vbx, target_energy=args.target_energy,
                                        first_pass_max_points=args.first_pass_max_points)
        labels = diarizer.cluster(embeddings)
    except ValueError as e:
        sys.exit(str(e))
    for reco, kept in diarizer.pca_report.items():
        log.info("[INFO] Recording %s: per-recording PCA: %s." % (reco, "%d of %d dimensions kept" % (kept, scorer.dim) if kept else "none, scored with the global model"))
    for reco, (before, after, iters, elbo) in diarizer.vbx_report.items():
        log.info("[INFO] Recording %s: VBx: %d speakers before, %d after, %d iterations, last ELBO %.6f." % (reco, before, after, iters, elbo))
    turns = {}
    for reco, lab in labels.items():
        turns[reco] = [(s * FRAME_SHIFT, e * FRAME_SHIFT, l) for s, e, l in diarization.rttm_turns(windows_of[reco], lab)]
        log.info("[INFO] Recording %s: %d speakers, %d turns." % (reco, int(lab.max()) + 1, len(turns[reco])))
    diarization.write_rttm(args.rttm_out, turns)
    trainer.close()


if __name__ == "__main__":
    main()
