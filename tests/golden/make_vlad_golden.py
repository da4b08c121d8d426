"""Generates tests/golden/vlad_golden.npz from the reference's own NumPy oracle model/test_utils.py:compute_ghost_vlad (the function the
reference's pooling self-test checks the TF graph against, model/pooling.py:478-510).

Run in the build container only (needs /root/reference):  python tests/golden/make_vlad_golden.py
The reference is read at run time, as make_attention_golden.py does; nothing of it is stored here.  Inputs: post-ReLU-like values, one
chunk times 100 where the batch has three or more; no residual is exactly zero (the reference's NumPy divides by the norm without an
epsilon and would give NaN there).
"""
import os
import sys
import types

import numpy as np

sys.path.insert(0, "/root/reference")
from model import test_utils  # noqa: E402

out = {}
rs = np.random.RandomState(20261020)
i = 0
for final in (False, True):
    for (b, l, d, k, g) in ((4, 13, 24, 3, 2), (3, 40, 10, 4, 0), (2, 1, 8, 2, 1)):
        value = rs.rand(b, l, d)
        if b > 2:
            value[2] *= 100.0
        key = rs.randn(b, l, k + g)
        centers = rs.randn(k + g, d) * 0.3
        params = types.SimpleNamespace(vlad_num_centers=k, vlad_num_ghosts=g, vlad_final_l2_norm=final)
        vlad = test_utils.compute_ghost_vlad(value, key, centers, params)
        assert np.all(np.isfinite(vlad))
        out["value_%d" % i], out["key_%d" % i], out["centers_%d" % i] = value, key, centers
        out["vlad_%d" % i], out["final_%d" % i], out["num_centers_%d" % i] = vlad, np.array(final), np.array(k)
        i += 1
out["num_cases"] = np.array(i)
path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "vlad_golden.npz")
np.savez_compressed(path, **out)
print("wrote %s (%d cases)" % (path, i))
