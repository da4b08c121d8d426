"""Writes tests/golden/triplet_golden.npz: inputs and the values of the reference's own NumPy oracles (model/test_utils.py:
compute_triplet_loss, {asoftmax,amsoftmax,arcsoftmax}_angular_triplet_loss, compute_ge2e_loss, pairwise_cos_similarity_np), executed here.

    python tests/golden/make_triplet_golden.py <checkout of the reference>

The reference is imported read-only; its functions modify their argument, so they get copies.  None of its text is stored: the file holds
embeddings, labels and the numbers the oracles returned.  Keys: "<case>/x", "<case>/labels", "<case>/shape" (speakers, segments, dim) and
"<case>/<configuration>" (names as tests/test_triplet_ref.py builds them).

Cases: `rand` embeddings (as the reference's self-test draws them) and mixed-sign `randn` ones at (speakers, segments, dim) = (4,3,16),
(5,2,8), (3,4,512), and the self-test's hostile rows (row 1 = row 0, row 2 = -row 0).  compute_triplet_loss normalises its rows first: the
stored x of a case is what was passed in, the test normalises the same way."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import triplet_ref as R  # noqa: E402

SHAPES = [(4, 3, 16), (5, 2, 8), (3, 4, 512)]
ANGULAR = [("asoftmax", 1.0), ("asoftmax", 2.0), ("asoftmax", 4.0), ("additive_margin_softmax", 0.1), ("additive_angular_margin_softmax", 0.3)]
SEMIHARD_MARGIN = 0.2


def configurations():
    """[(name, kind, options)] in one order for the generator and the test"""
    out = [("semihard/squared=%d" % sq, R.SEMIHARD, dict(margin=SEMIHARD_MARGIN, squared=bool(sq))) for sq in (1, 0)]
    for tt in (R.ALL, R.HARD):
        for lt, m in ANGULAR:
            out.append(("angular/%s/%s/%g" % (tt, lt, m), tt, dict(margin=m, margin_kind=R.MARGIN_KINDS[lt])))
    return out


def normalized(x):
    x = R.f64(x)
    return x / np.sqrt((x * x).sum(axis=1, keepdims=True))


def stable(case):
    x, labels = case
    for name, kind, opt in configurations():
        xin = normalized(x) if kind == R.SEMIHARD else x
        if not R.pair_loss(xin, labels, kind, backward=False, **opt).gap >= R.STABLE:
            return False
    return True


def cases():
    out = {}
    for sign in ("rand", "randn"):
        for n, m, d in SHAPES:
            seed, (x, labels) = R.stable_case(lambda s: R.embeddings(n, m, d, s, sign), stable)
            out["%s_%dx%dx%d_seed%d" % (sign, n, m, d, seed)] = (x, labels, (n, m, d))
    x, labels = R.embeddings(4, 3, 16, 0, "randn")
    x[1], x[2] = x[0], -x[0]
    out["hostile_4x3x16"] = (x, labels, (4, 3, 16))
    return out


def main(ref_root):
    sys.path.insert(0, ref_root)
    from model import test_utils as T
    oracle = {"asoftmax": T.asoftmax_angular_triplet_loss, "additive_margin_softmax": T.amsoftmax_angular_triplet_loss,
              "additive_angular_margin_softmax": T.arcsoftmax_angular_triplet_loss}
    blob = {}
    for case, (x, labels, shape) in sorted(cases().items()):
        blob[case + "/x"], blob[case + "/labels"], blob[case + "/shape"] = x, labels, np.asarray(shape, np.int32)
        x64 = R.f64(x)
        for sq in (1, 0):
            blob["%s/semihard/squared=%d" % (case, sq)] = np.float64(T.compute_triplet_loss(x64.copy(), labels.copy(), SEMIHARD_MARGIN, bool(sq)))
        for tt in (R.ALL, R.HARD):
            for lt, m in ANGULAR:
                blob["%s/angular/%s/%s/%g" % (case, tt, lt, m)] = np.float64(oracle[lt](x64.copy(), labels.copy(), m, tt))
        blob[case + "/e2e"] = np.float64(T.compute_ge2e_loss(x64.copy(), labels.copy(), 20.0, 0.0, "softmax"))
        blob[case + "/cos"] = np.asarray(T.pairwise_cos_similarity_np(x64.copy()), np.float64)
    np.savez_compressed(os.path.join(HERE, "triplet_golden.npz"), **blob)
    print("wrote %d arrays for %d cases" % (len(blob), len(cases())))


if __name__ == "__main__":
    main(sys.argv[1])
