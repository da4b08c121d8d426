#!/usr/bin/env python3
"""Cosine scoring of a trial list on the GPU, with optional centring and adaptive symmetric score normalisation (AS-norm):

    python nnet/lib/score.py [-g GPU] [--center-on RSPECIFIER] [--cohort RSPECIFIER --top-k N] trials enrol_rspecifier test_rspecifier scores_out

The stage behind extract.py, for which the reference recipe goes to Kaldi (egs/voxceleb/v1/run.sh, cosine back end: ivector-mean,
ivector-subtract-global-mean | ivector-normalize-length, ivector-compute-dot-products, compute-eer).  The rspecifiers name float-vector
tables as extract.py writes them (`ark:FILE` or `scp:FILE`); enrol_rspecifier == test_rspecifier (VoxCeleb) is read and prepared once.
--center-on: the mean of that table, accumulated once on the host in fp64, is subtracted from every vector, cohort included.
--cohort: every score s becomes 0.5 * ((s - mu_e) / sigma_e + (s - mu_t) / sigma_t), mu / sigma the mean and deviation of the --top-k
largest scores of the enrolment / test vector against the cohort vectors.
Output: `enrol test score` lines in trial order.  A trial whose key is missing from its table is logged and skipped; the number skipped is
logged at the end.  When every kept trial carries a label, EER, minDCF08 and minDCF10 are logged.
Not here: LDA / PLDA, multi-utterance enrolment (spk2utt averaging), DET plots.
"""
import sys

import numpy as np

import _cli
from misc import scoring


def main():
    log = _cli.logger()
    args = _cli.parser_for("gpu", "center_on", "cohort", "top_k", "trials", "enrol_rspecifier", "test_rspecifier", "scores_out").parse_args()
    if args.cohort and args.top_k <= 0:
        sys.exit("--top-k must be positive (got %d)" % args.top_k)
    import torch
    device = "cuda:%d" % (args.gpu % max(torch.cuda.device_count(), 1) if args.gpu >= 0 else 0)
    trials = scoring.read_trials(args.trials)
    enrol_keys, enrol = scoring.read_vectors(args.enrol_rspecifier)
    same = args.test_rspecifier == args.enrol_rspecifier
    test_keys, test = (enrol_keys, enrol) if same else scoring.read_vectors(args.test_rspecifier)
    d = enrol.shape[1]
    tables = [("test_rspecifier", test)]
    center = cohort = None
    if args.center_on:
        center = scoring.read_vectors(args.center_on)[1]
        tables.append(("--center-on", center))
    if args.cohort:
        cohort = scoring.read_vectors(args.cohort)[1]
        tables.append(("--cohort", cohort))
    for name, table in tables:
        if table.shape[1] != d:
            sys.exit("dimension mismatch: enrol_rspecifier holds vectors of %d dimensions, %s of %d" % (d, name, table.shape[1]))
    kept, ei, ti, skipped = scoring.index_trials(trials, enrol_keys, test_keys)
    for a, b, _ in skipped:
        log.info("[INFO] Trial %s %s: %s, skip." % (a, b, "no vector for a key"))
    scores = np.zeros(0, np.float32)
    if kept:
        scorer = scoring.CosineScorer(device, center=None if center is None else scoring.center_mean(center))
        e_prep = scorer.prepare(enrol)
        t_prep = e_prep if same else scorer.prepare(test)
        if cohort is not None:
            scorer.cohort(cohort, args.top_k)
        scores = scorer.score(e_prep, t_prep, ei, ti)
    with open(args.scores_out, "w") as f:
        f.write("".join("%s %s %.6f\n" % (a, b, s) for (a, b, _), s in zip(kept, scores)))
    log.info("[INFO] Scored %d trials, skipped %d." % (len(kept), len(skipped)))
    if kept and all(label is not None for _, _, label in kept):
        targets = np.asarray([label for _, _, label in kept])
        if targets.any() and not targets.all():
            log.info("[INFO] EER %.4f%%  minDCF08 %.4f  minDCF10 %.4f" % (
                100.0 * scoring.compute_eer(scores, targets.astype(np.float64)),
                scoring.compute_min_dcf(scores, targets, *scoring.MIN_DCF_PRESETS["minDCF08"]),
                scoring.compute_min_dcf(scores, targets, *scoring.MIN_DCF_PRESETS["minDCF10"])))


if __name__ == "__main__":
    main()
