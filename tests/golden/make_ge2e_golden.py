"""Writes tests/golden/ge2e_golden.npz: the values of the reference's own NumPy statement of the GE2E loss (model/test_utils.py:21-86,
compute_ge2e_loss), executed here, for both loss types and (w, b) in ge2e_ref.WB on the cases of make_triplet_golden.py - `rand`, mixed-sign
and hostile embeddings.

    python tests/golden/make_ge2e_golden.py <checkout of the reference>

The reference is imported read-only; its function modifies its argument, so it gets copies.  None of its text is stored: the file holds
embeddings, shapes and the numbers the oracle returned.  Keys: "<case>/x", "<case>/shape" (speakers, segments, dim) and
"<case>/<type>/<w>/<b>" (ge2e_key)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import ge2e_ref as G  # noqa: E402
import make_triplet_golden as MT  # noqa: E402
import triplet_ref as R  # noqa: E402


def ge2e_key(case, loss_type, w, b):
    return "%s/%s/%g/%g" % (case, loss_type, w, b)


def main(ref_root):
    sys.path.insert(0, ref_root)
    from model import test_utils as T
    blob = {}
    cases = MT.cases()
    for case, (x, labels, shape) in sorted(cases.items()):
        blob[case + "/x"], blob[case + "/shape"] = x, np.asarray(shape, np.int32)
        for loss_type in G.TYPES:
            for w, b in G.WB:
                blob[ge2e_key(case, loss_type, w, b)] = np.float64(T.compute_ge2e_loss(R.f64(x).copy(), labels.copy(), w, b, loss_type))
    np.savez_compressed(os.path.join(HERE, "ge2e_golden.npz"), **blob)
    print("wrote %d arrays for %d cases" % (len(blob), len(cases)))


if __name__ == "__main__":
    main(sys.argv[1])
