#!/usr/bin/env python3
"""Scoring of a trial list on the GPU: cosine with optional centring and adaptive symmetric score normalisation (AS-norm), or behind a
trained LDA / PLDA back end, with optional multi-utterance enrolment:

    python nnet/lib/score.py [-g GPU] [--center-on RSPECIFIER] [--cohort RSPECIFIER --top-k N]
                             [--backend DIR --scoring {cosine,lda_cos,plda,plda_asnorm}] [--enrol-spk2utt FILE]
                             trials enrol_rspecifier test_rspecifier scores_out

The stage behind extract.py, for which the reference recipe goes to Kaldi (egs/voxceleb/v1/run.sh, cosine back end: ivector-mean,
ivector-subtract-global-mean | ivector-normalize-length, ivector-compute-dot-products, compute-eer).  The rspecifiers name float-vector
tables as extract.py writes them (`ark:FILE` or `scp:FILE`); enrol_rspecifier == test_rspecifier (VoxCeleb) is read and prepared once.
--center-on: the mean of that table, accumulated once on the host in fp64, is subtracted from every vector, cohort included.
--cohort: every score s becomes 0.5 * ((s - mu_e) / sigma_e + (s - mu_t) / sigma_t), mu / sigma the mean and deviation of the --top-k
largest scores of the enrolment / test vector against the cohort vectors.
Output: `enrol test score` lines in trial order.  A trial whose key is missing from its table is logged and skipped; the number skipped is
logged at the end.  When every kept trial carries a label, EER, minDCF08 and minDCF10 are logged.
--backend DIR (nnet/lib/train_backend.py wrote it) with --scoring lda_cos | plda: every vector is centred on the back end's mean.vec (giving
--center-on as well is refused), taken through transform.mat and length-normalised (run.sh stage 10-11: ivector-subtract-global-mean |
transform-vec | ivector-normalize-length); lda_cos scores the cosine, plda the log-likelihood ratio of ivector-plda-scoring
--normalize-length=true.  --scoring plda_asnorm (needs --backend and --cohort; honours --top-k): the PLDA ratios AS-normalised, mu / sigma
the statistics of the --top-k largest ratios of the enrolment model (with its utterance count) / of the test vector (as a one-utterance model)
against the cohort vectors.  --scoring plda with --cohort is refused: the normalised scores have a name of their own.
--enrol-spk2utt FILE (any scoring mode): a model is the plain average of its speaker's raw enrolment vectors (ivector-mean ark:spk2utt), the
trials name speakers on the enrol side, and with plda the number of utterances enters the score (--num-utts).
Without the three new options the output is what it was before they existed, byte for byte.
Not here: DET plots.  (ivector-adapt-plda: nnet/lib/adapt_backend.py.)
"""
import sys

import numpy as np

import _cli
from misc import scoring


def backend_scores(args, log, device, trials, enrol_keys, enrol, test_keys, test, same, center, cohort):
    """The paths the options --backend and --enrol-spk2utt open: (scores, kept trials, skipped trials)."""
    from misc import backend as B
    be = B.Backend.load(args.backend) if args.backend else None
    if be is not None and be.d != enrol.shape[1]:
        sys.exit("dimension mismatch: enrol_rspecifier holds vectors of %d dimensions, the back end %s works on %d" % (enrol.shape[1], args.backend, be.d))
    if be is None:      # cosine on averaged models: a back end that only centres
        be = B.Backend(np.zeros(enrol.shape[1], np.float32) if center is None else scoring.center_mean(center).astype(np.float32))
    plda = args.scoring in ("plda", "plda_asnorm")
    if plda and be.plda is None:
        sys.exit("--scoring %s: the back end %s holds no plda file" % (args.scoring, args.backend))
    scorer = B.BackendScorer(be, "plda" if plda else "lda_cos", device)
    model_keys, models, counts = enrol_keys, enrol, None
    if args.enrol_spk2utt:
        model_keys, models, counts = scorer.enrol_average(enrol, enrol_keys, B.read_spk2utt(args.enrol_spk2utt), log)
    same = same and not args.enrol_spk2utt
    kept, ei, ti, skipped = scoring.index_trials(trials, model_keys, model_keys if same else test_keys)
    for a, b, _ in skipped:
        log.info("[INFO] Trial %s %s: %s, skip." % (a, b, "no vector for a key"))
    if not kept:
        return np.zeros(0, np.float32), kept, skipped
    e_prep = scorer.prepare(models, n_utts=counts if plda else None)
    t_prep = e_prep if same else scorer.prepare(test)
    if plda:
        if args.scoring == "plda_asnorm":
            scorer.cohort(cohort, args.top_k)
        return scorer.score(e_prep, t_prep, ei, ti, enrol_n=counts), kept, skipped
    if cohort is None:
        return scorer.score(e_prep, t_prep, ei, ti), kept, skipped
    # AS-norm behind the chain: the prepared tables are unit-length rows on a zero-padded pitch, what CosineScorer works on
    cos = scoring.CosineScorer(device)
    cos.d = be.dim
    cos._cohort, cos.top_k = scorer.prepare(cohort), args.top_k
    return cos.score(e_prep, t_prep, ei, ti), kept, skipped


def main():
    log = _cli.logger()
    args = _cli.parser_for("gpu", "center_on", "cohort", "top_k", "backend", "scoring", "enrol_spk2utt", "trials", "enrol_rspecifier",
                           "test_rspecifier", "scores_out").parse_args()
    if args.cohort and args.top_k <= 0:
        sys.exit("--top-k must be positive (got %d)" % args.top_k)
    if args.scoring != "cosine" and not args.backend:
        sys.exit("--scoring %s needs --backend DIR (a directory written by train_backend.py)" % args.scoring)
    if args.backend and args.scoring == "cosine":
        sys.exit("--backend is given but --scoring is cosine: choose --scoring lda_cos or plda")
    if args.backend and args.center_on:
        sys.exit("--backend and --center-on exclude each other: with a back end the centre is its mean.vec")
    if args.scoring == "plda" and args.cohort:
        sys.exit("--cohort with --scoring plda is not supported: plda writes raw log-likelihood ratios; --scoring plda_asnorm normalises them against the cohort")
    if args.scoring == "plda_asnorm" and not args.cohort:
        sys.exit("--scoring plda_asnorm needs --cohort RSPECIFIER (the vectors the PLDA scores are normalised against)")
    device = _cli.device(args.gpu)
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
    if args.backend or args.enrol_spk2utt:
        scores, kept, skipped = backend_scores(args, log, device, trials, enrol_keys, enrol, test_keys, test, same, center, cohort)
    else:
        kept, ei, ti, skipped = scoring.index_trials(trials, enrol_keys, test_keys)
        for a, b, _ in skipped:
            log.info("[INFO] Trial %s %s: %s, skip." % (a, b, "no vector for a key"))
        scores = np.zeros(0, np.float32)
    if kept and not (args.backend or args.enrol_spk2utt):
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
