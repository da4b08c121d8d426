#!/usr/bin/env python3
"""The clustering threshold of diarize.py, tuned on a development set: what Kaldi's callhome_diarization/v2 recipe does when it sweeps
thresholds on one fold, scores each with md-eval.pl -c 0.25 and applies the best to the other fold - restated; nothing is compared with a
run of Kaldi or of md-eval:

    python nnet/lib/tune_diarization.py [-g GPU] [--backend DIR --scoring {cosine,lda_cos,plda} [--target-energy F]]
                                        --thresholds "-0.3:0.05:0.3" | "a,b,c" [--collar 0.25] [--overlap {score,ignore,first}]
                                        [--vbx [--vbx-fa LIST --vbx-fb LIST --vbx-loop-prob LIST --vbx-max-iters 20 --vbx-epsilon 1e-4 --vbx-init-smoothing 5]]
                                        [--first-pass-max-points 2048] --ref-rttm FILE embeddings_rspecifier out_dir

embeddings_rspecifier: the windows' embeddings that diarize.py --write-embeddings writes; their keys `recording-startframe-endframe`
carry the windows, so neither the network nor the features are needed.  The recordings are scored and clustered ONCE, down to one
cluster (misc/diarization.py Diarizer.sweep: the clusterer's merge log holds the labels of every threshold as a prefix, xv_ahc_cut reads
them off: DESIGN.md section 6n); the error of every threshold against --ref-rttm is counted on the device (DerSweep, xv_diar_confusion):
10 ms frames, --collar seconds around every reference boundary not scored, overlapped reference speech by --overlap, the speakers mapped
one to one for the largest matched time.  With --vbx the grid is the thresholds times the listed --vbx-fa / --vbx-fb / --vbx-loop-prob
values, each point through xv_vbx behind the cut.
Output: out_dir/der_table.txt, one line per grid point - miss, false alarm, speaker error and DER in percent of the scored reference speaker
time, pooled over the recordings, or `not counted` with the reason -, and out_dir/threshold: the best point's threshold, with --vbx followed
by its `--vbx --vbx-fa A --vbx-fb B --vbx-loop-prob P`, so that `diarize.py --threshold $(cat out_dir/threshold) ...` applies it.  A tie goes
to the lower threshold (then to the earlier VBx entry); the best point is logged.
Refused: what diarize.py refuses of --backend / --scoring / --vbx / --target-energy / --first-pass-max-points, a --thresholds that is
neither form (or a step that is not positive, a last below the first, a NaN), a negative --collar, a key that is not
`recording-start-end`, a recording of --ref-rttm without embeddings and the reverse, a grid without a counted point.
"""
import os
import sys

import numpy as np

import _cli
import _lib      # (the caps of the kernels: no device library loads)
from misc import diarization

FRAME_SHIFT = 0.01      # seconds per frame of the windows in the keys


def parse_thresholds(text):
    """`first:step:last` -> first + i * step for i = 0 .. round((last - first) / step), both ends included and no step added to a step; or
    `a,b,c` -> those.  ValueError names what is wrong."""
    try:
        if ":" in text:
            first, step, last = (float(v) for v in text.split(":"))
            if not (step > 0 and last >= first):      # (a NaN fails either comparison)
                raise ValueError
            count = int(round((last - first) / step))
            if abs(first + count * step - last) > 1e-9 * max(1.0, abs(first), abs(last)):
                raise ValueError
            values = [first + i * step for i in range(count)] + [last]
        else:
            values = [float(v) for v in text.split(",")]
        if not values or any(v != v for v in values):
            raise ValueError
    except ValueError:
        raise ValueError("--thresholds must be `first:step:last` with a positive step that leads from first to last, or `a,b,c` (got %r)" % text)
    return values


def parse_list(text, flag):
    try:
        return [float(v) for v in text.split(",")]
    except ValueError:
        raise ValueError("%s must be a list of numbers `a,b,c` (got %r)" % (flag, text))


def window_of(key):
    """`recording-startframe-endframe` -> (recording, start, end)."""
    parts = key.rsplit("-", 2)
    if len(parts) != 3 or not (parts[1].isdigit() and parts[2].isdigit()) or int(parts[2]) <= int(parts[1]) or not parts[0]:
        raise ValueError("key %s is not `recording-startframe-endframe` (the embeddings diarize.py --write-embeddings writes)" % key)
    return parts[0], int(parts[1]), int(parts[2])


def join_option_values(argv, flags=("--thresholds",)):
    """`--thresholds -0.3:0.05:0.3` -> `--thresholds=-0.3:0.05:0.3`: argparse takes a value that starts with `-` and is no number for an option."""
    out, i = [], 0
    while i < len(argv):
        if argv[i] in flags and i + 1 < len(argv):
            out.append(argv[i] + "=" + argv[i + 1])
            i += 2
        else:
            out.append(argv[i])
            i += 1
    return out


def main(argv=None):
    log = _cli.logger()
    args = _cli.parser_for("gpu", "backend", "diar_scoring", "target_energy", "thresholds", "collar", "overlap", "vbx", "vbx_fa_list", "vbx_fb_list",
                           "vbx_loop_prob_list", "vbx_max_iters", "vbx_epsilon", "vbx_init_smoothing", "first_pass_max_points", "ref_rttm",
                           "embeddings_rspecifier", "tune_out_dir").parse_args(join_option_values(sys.argv[1:] if argv is None else argv))
    if args.scoring != "cosine" and not args.backend:
        sys.exit("--scoring %s needs --backend DIR (a directory written by train_backend.py)" % args.scoring)
    if args.backend and args.scoring == "cosine":
        sys.exit("--backend is given but --scoring is cosine: choose --scoring lda_cos or plda")
    if args.vbx and args.scoring != "plda":
        sys.exit("--vbx needs --scoring plda (VBx models the windows in the PLDA space of --backend), not --scoring %s" % args.scoring)
    try:
        thresholds = parse_thresholds(args.thresholds)
        fa, fb, loop = (parse_list(v, flag) for v, flag in ((args.vbx_fa, "--vbx-fa"), (args.vbx_fb, "--vbx-fb"), (args.vbx_loop_prob, "--vbx-loop-prob")))
    except ValueError as e:
        sys.exit(str(e))
    if args.vbx and not (all(0.0 < p < 1.0 for p in loop) and all(v > 0 for v in fa + fb) and 1 <= args.vbx_max_iters <= _lib.VBX_MAX_ITERS
                         and args.vbx_init_smoothing >= 0 and args.vbx_epsilon == args.vbx_epsilon):
        sys.exit("--vbx: --vbx-loop-prob must lie strictly between 0 and 1, --vbx-fa and --vbx-fb be positive, --vbx-max-iters lie in 1 .. %d, "
                 "--vbx-init-smoothing not be negative" % _lib.VBX_MAX_ITERS)
    if args.target_energy is not None and args.scoring != "plda":
        sys.exit("--target-energy needs --scoring plda (the per-recording PCA projects the PLDA model of --backend), not --scoring %s" % args.scoring)
    if args.target_energy is not None and not 0.0 < args.target_energy <= 1.0:
        sys.exit("--target-energy must lie in (0, 1] (got %g)" % args.target_energy)
    if not 2 <= args.first_pass_max_points <= diarization.FIRST_PASS_CAP:
        sys.exit("--first-pass-max-points must lie in 2 .. %d (got %d)" % (diarization.FIRST_PASS_CAP, args.first_pass_max_points))
    if not args.collar >= 0.0:
        sys.exit("--collar must not be negative (got %g)" % args.collar)
    if not args.ref_rttm:
        sys.exit("--ref-rttm FILE is needed: the reference the thresholds are scored against")
    # (the refusals above come before the imports that load the device libraries)
    from misc import scoring
    try:
        reference = diarization.read_rttm(args.ref_rttm)
        keys, matrix = scoring.read_vectors(args.embeddings_rspecifier)
        rows, windows = {}, {}
        for i, key in enumerate(keys):
            reco, start, end = window_of(key)
            rows.setdefault(reco, []).append(i)
            windows.setdefault(reco, []).append((start * FRAME_SHIFT, end * FRAME_SHIFT))
    except ValueError as e:
        sys.exit(str(e))
    for reco in reference:
        if reco not in rows:
            sys.exit("recording %s of %s has no embeddings in %s" % (reco, args.ref_rttm, args.embeddings_rspecifier))
    for reco in rows:
        if reco not in reference:
            sys.exit("recording %s of %s has no turn in %s" % (reco, args.embeddings_rspecifier, args.ref_rttm))
    embeddings = {reco: matrix[idx] for reco, idx in rows.items()}
    device = _cli.device(args.gpu)
    try:
        if args.backend:
            from misc import backend as B
            be = B.Backend.load(args.backend)
            if be.d != matrix.shape[1]:
                sys.exit("dimension mismatch: the embeddings have %d dimensions, the back end %s works on %d" % (matrix.shape[1], args.backend, be.d))
            if args.scoring == "plda" and be.plda is None:
                sys.exit("--scoring plda: the back end %s holds no plda file" % args.backend)
            scorer = B.BackendScorer(be, args.scoring, device)
        else:
            scorer = scoring.CosineScorer(device)
        grid = None
        if args.vbx:
            grid = [diarization.VbxOptions(fa=a, fb=b, loop_prob=p, max_iters=args.vbx_max_iters, epsilon=args.vbx_epsilon, init_smoothing=args.vbx_init_smoothing)
                    for a in fa for b in fb for p in loop]
        diarizer = diarization.Diarizer(scorer, threshold=thresholds[0], vbx=grid[0] if grid else None, target_energy=args.target_energy,
                                        first_pass_max_points=args.first_pass_max_points)
        labels = diarizer.sweep(embeddings, thresholds, vbx_grid=grid)
        der = diarization.DerSweep(device, {reco: reference[reco] for reco in rows}, windows, collar=args.collar, overlap=args.overlap)
        # (one table over the whole grid: its points as cuts, the VBx entries outermost)
        table = der.score({reco: lab.reshape(-1, lab.shape[-1]) for reco, lab in labels.items()})
    except ValueError as e:
        sys.exit(str(e))
    os.makedirs(args.out_dir, exist_ok=True)
    best, lines = None, []
    for k in range(len(thresholds) * len(grid or [None])):
        opt, threshold = (grid[k // len(thresholds)] if grid else None), thresholds[k % len(thresholds)]
        point = "threshold %r" % threshold + (" fa %r fb %r loop_prob %r" % (opt.fa, opt.fb, opt.loop_prob) if opt else "")
        pooled = table.pooled(k)
        if pooled is None:
            lines.append("%s not counted: %s" % (point, table.why_not(k)))
            continue
        lines.append("%s miss %.2f fa %.2f error %.2f DER %.2f" % ((point,) + tuple(100.0 * v for v in pooled)))
        errors = int(table.miss[k].sum() + table.fa[k].sum() + table.error[k].sum())      # (integers: a tie is a tie)
        if best is None or (errors, threshold) < best[:2]:
            best = (errors, threshold, k, opt, lines[-1])
    with open(os.path.join(args.out_dir, "der_table.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    if best is None:
        sys.exit("no point of the grid was counted (see %s)" % os.path.join(args.out_dir, "der_table.txt"))
    _, threshold, _, opt, line = best
    with open(os.path.join(args.out_dir, "threshold"), "w") as f:
        f.write(repr(threshold) + (" --vbx --vbx-fa %r --vbx-fb %r --vbx-loop-prob %r" % (opt.fa, opt.fb, opt.loop_prob) if opt else "") + "\n")
    log.info("[INFO] %d recordings, %d grid points; the best: %s." % (len(rows), len(lines), line))


if __name__ == "__main__":
    main()
