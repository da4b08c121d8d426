#!/usr/bin/env python3
"""Adapt a trained LDA / PLDA back end to an unlabelled in-domain table of embeddings, on the GPU:

    python nnet/lib/adapt_backend.py [-g GPU] [--within-covar-scale 0.3] [--between-covar-scale 0.7] [--mean-diff-scale 1.0]
                                     [--mean-only {true,false}] backend_in adapt_rspecifier backend_out

What the SRE recipe goes to Kaldi for behind train_backend.py (egs/sre/v1/run.sh:451-492): ivector-mean of the in-domain table (the new
mean.vec), the out-of-domain transform.mat kept, and ivector-adapt-plda --within-covar-scale=0.75 --between-covar-scale=0.25 on the in-domain
vectors centred on that mean, transformed and length-normalised.  backend_out receives mean.vec, transform.mat (copied) and plda, which
nnet/lib/score.py --backend reads.  --mean-only true writes the recipe's other system: the out-of-domain PLDA on the in-domain mean
(run.sh:477-483), nothing adapted.
The statistics of the adaptation vectors (the transform chain, their scatter matrix and their sum) run on the GPU; the estimator runs on
the host in fp64 (misc/backend.py adapt_plda).  N, the number of eigenvalues above 1 and their range are logged.
Refused by name: a backend_in without a plda file (unless --mean-only true), a dimension mismatch, negative scales, backend_out == backend_in.
"""
import os
import sys

import _cli
from misc import backend, scoring


def main():
    log = _cli.logger()
    args = _cli.parser_for("gpu", "within_covar_scale", "between_covar_scale", "mean_diff_scale", "mean_only", "backend_in", "adapt_rspecifier",
                           "backend_out").parse_args()
    for name in ("within_covar_scale", "between_covar_scale", "mean_diff_scale"):
        if getattr(args, name) < 0:
            sys.exit("--%s must not be negative (got %g)" % (name.replace("_", "-"), getattr(args, name)))
    if os.path.realpath(args.backend_out) == os.path.realpath(args.backend_in):      # (realpath: a link to backend_in is backend_in)
        sys.exit("backend_out == backend_in (%s): the adapted back end goes to a directory of its own" % args.backend_in)
    mean_only = args.mean_only == "true"
    try:
        model = backend.Backend.load(args.backend_in)
    except ValueError as e:
        sys.exit(str(e))
    if model.plda is None and not mean_only:
        sys.exit("the back end %s holds no plda file: nothing to adapt (--mean-only true replaces the mean alone)" % args.backend_in)
    _, matrix = scoring.read_vectors(args.adapt_rspecifier)
    if matrix.shape[1] != model.d:
        sys.exit("dimension mismatch: adapt_rspecifier holds vectors of %d dimensions, the back end %s works on %d" % (matrix.shape[1], args.backend_in, model.d))
    if mean_only:
        out = model.recentred(matrix)
        log.info("[INFO] Mean of N = %d vectors; transform.mat and plda are copied." % matrix.shape[0])
    else:
        device = _cli.device(args.gpu)
        out = model.adapt(matrix, device=device, within_covar_scale=args.within_covar_scale, between_covar_scale=args.between_covar_scale,
                          mean_diff_scale=args.mean_diff_scale, log=log)
    out.save(args.backend_out)
    log.info("[INFO] Back end written to %s." % args.backend_out)


if __name__ == "__main__":
    main()
