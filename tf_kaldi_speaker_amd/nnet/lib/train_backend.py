#!/usr/bin/env python3
"""Train the LDA / PLDA back end on a table of embeddings, on the GPU:

    python nnet/lib/train_backend.py [-g GPU] [--lda-dim 200] [--no-lda] [--num-em-iters 10] train_rspecifier spk2utt out_dir

What the reference recipes go to Kaldi for behind extract.py (egs/voxceleb/v1/run.sh:370-401, egs/sre/v1/run.sh:397-490): ivector-mean,
ivector-compute-lda --total-covariance-factor=0.0 --dim=N on the centred vectors, ivector-compute-plda on the centred, transformed,
length-normalised ones.  train_rspecifier names a float-vector table as extract.py writes it (`ark:FILE` or `scp:FILE`), spk2utt groups its
keys by speaker; an utterance without a vector is logged and skipped, a speaker without any is logged and dropped.  out_dir receives the
recipe's files: mean.vec, transform.mat (not with --no-lda) and plda, which nnet/lib/score.py --backend reads.
The statistics that grow with the corpus (scatter matrices, per-speaker means, the transform chain) run on the GPU; the
eigendecompositions and the EM run on the host in fp64 (misc/backend.py).  N, K, the kept LDA eigenvalue range and the PLDA's psi range are
logged.
Domain adaptation of the trained model (ivector-adapt-plda): nnet/lib/adapt_backend.py.
"""
import sys

import _cli
from misc import backend, scoring


def main():
    log = _cli.logger()
    args = _cli.parser_for("gpu", "lda_dim", "no_lda", "num_em_iters", "train_rspecifier", "spk2utt", "out_dir").parse_args()
    if not args.no_lda and args.lda_dim <= 0:
        sys.exit("--lda-dim must be positive (got %d); --no-lda trains without an LDA" % args.lda_dim)
    if args.num_em_iters <= 0:
        sys.exit("--num-em-iters must be positive (got %d)" % args.num_em_iters)
    device = _cli.device(args.gpu)
    keys, matrix = scoring.read_vectors(args.train_rspecifier)
    if not args.no_lda and args.lda_dim > matrix.shape[1]:
        sys.exit("--lda-dim %d exceeds the %d dimensions of the vectors" % (args.lda_dim, matrix.shape[1]))
    model = backend.Backend.train(matrix, keys, backend.read_spk2utt(args.spk2utt), lda_dim=None if args.no_lda else args.lda_dim,
                                  device=device, num_em_iters=args.num_em_iters, log=log)
    model.save(args.out_dir)
    log.info("[INFO] Back end written to %s." % args.out_dir)


if __name__ == "__main__":
    main()
