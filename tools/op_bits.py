#!/usr/bin/env python3
"""The bits of every op of the scoring and back-end units (xv_score.hip, xv_backend.hip, xv_backend_cohort.hip), of ops.vbx and of
ops.backend_pca_plda on seeded inputs at fixed shapes: one line `op  shape  sha256(output bytes)` each.  These ops promise the same bits every time, so the output of two
builds of the library (XV_LIB=<another build> python3 tools/op_bits.py) must not differ in any line.  Needs the GPU."""
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from tf_kaldi_speaker_amd import ops                      # noqa: E402
from tf_kaldi_speaker_amd.misc import backend as B        # noqa: E402
from tests import pca_plda_ref, vbx_ref                   # noqa: E402

rs = np.random.RandomState(20240)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def rnd(*shape):
    return dev(rs.randn(*shape).astype(np.float32))


def show(op, shape, *outs):
    h = hashlib.sha256()
    for o in outs:
        h.update(o.detach().cpu().contiguous().numpy().tobytes())
    print("%-28s %-44s %s" % (op, shape, h.hexdigest()), flush=True)


def padded(x, d):      # x's columns in a buffer on the pitch d rounded up to 4, the padding not zero: the operand of an in-place call
    buf = torch.full((x.shape[0], (d + 3) // 4 * 4), 7.0, device="cuda")
    buf[:, :d] = x
    return buf


def tables(d, counts):
    psi = np.sort(rs.uniform(0.05, 5.0, d))[::-1].copy()
    return dev(psi.astype(np.float32)), tuple(dev(a) for a in B.plda_coefficients(psi, counts))


def row_ops():
    for d in (30, 200, 512, 601):
        psi, (coef, g, k0) = tables(d, [1, 3, 8])
        _, (coef1, g1, k01) = tables(d, [1])
        for rows in (1, 5, 129):
            x, mean, tag = rnd(rows, d), rnd(d), "d=%d rows=%d" % (d, rows)
            n_utts = rs.choice([1, 3, 8], rows)
            for m, mt in ((None, ""), (mean, " mean")):
                for name, op in (("score_prepare", ops.score_prepare), ("backend_center", ops.backend_center)):
                    show(name, tag + mt, op(x, mean=m))
                    buf = padded(x, d)
                    show(name, tag + mt + " in place", op(buf, d, mean=m, out=buf))
            for n, nt in ((None, ""), (n_utts, " n_utts")):
                show("backend_plda_normalize", tag + nt, ops.backend_plda_normalize(x, d, psi, n_utts=n))
                buf = padded(x, d)
                show("backend_plda_normalize", tag + nt + " in place", ops.backend_plda_normalize(buf, d, psi, n_utts=n, out=buf))
            e, t = ops.score_prepare(x, mean=mean), ops.score_prepare(rnd(7, d))
            ei, ti = rs.randint(0, rows, 131), rs.randint(0, 7, 131)
            e_stats, t_stats = ops.score_cohort_stats(e, t, d, 3), ops.score_cohort_stats(t, t, d, 3)
            show("score_trials", tag, ops.score_trials(e, t, d, ei, ti))
            show("score_trials", tag + " stats", ops.score_trials(e, t, d, ei, ti, e_stats, t_stats))
            show("score_normalize", tag, ops.score_normalize(rnd(131), ei, ti, e_stats, t_stats))
            u, v = ops.backend_plda_normalize(x, d, psi, n_utts=n_utts), ops.backend_plda_normalize(rnd(7, d), d, psi)
            show("backend_plda_trials", tag + " nidx", ops.backend_plda_trials(u, v, d, ei, ti, np.searchsorted([1, 3, 8], n_utts), coef, g, k0))
            show("backend_plda_trials", tag, ops.backend_plda_trials(u, v, d, ei, ti, np.zeros(rows, np.int64), coef1, g1, k01))
            offsets = np.unique(np.r_[0, rs.randint(1, rows + 1, 3), rows])
            show("backend_group_means", tag, *ops.backend_group_means(x, d, offsets, rs.permutation(rows)))
            show("backend_scatter", tag, ops.backend_scatter(x))
            show("backend_scatter", tag + " mean", ops.backend_scatter(x, mean=mean))


def cohort_ops():
    d = 200
    psi, (coef, g, k0) = tables(d, [1, 3, 8])
    _, (coef1, g1, k01) = tables(d, [1])
    for n_cohort in (5, 257, 1031):
        cohort, pc = ops.score_prepare(rnd(n_cohort, d)), ops.backend_plda_normalize(rnd(n_cohort, d), d, psi)
        for rows in (1, 130):
            raw, tag = rnd(rows, d), "n_cohort=%d rows=%d" % (n_cohort, rows)
            x, n_utts = ops.score_prepare(raw), rs.choice([1, 3, 8], rows)
            for ws, wt in ((None, ""), (ops.score_cohort_workspace_bytes(1, n_cohort, d), " one tile")):
                show("score_cohort_stats", tag + wt, ops.score_cohort_stats(x, cohort, d, 40, ws_bytes=ws))
            u3, u1 = ops.backend_plda_normalize(raw, d, psi, n_utts=n_utts), ops.backend_plda_normalize(raw, d, psi)
            for nq, u, nidx, tabs in ((1, u1, None, (coef1, g1, k01)), (3, u3, np.searchsorted([1, 3, 8], n_utts), (coef, g, k0))):
                for ws, wt in ((None, ""), (ops.backend_plda_cohort_workspace_bytes(1, n_cohort, d, nq), " one tile")):
                    show("backend_plda_cohort_stats", "%s n_distinct=%d%s" % (tag, nq, wt),
                         ops.backend_plda_cohort_stats(u, pc, d, nidx, *tabs, 40, ws_bytes=ws))


def dense_ops():
    for d in (30, 200):
        psi, tabs = tables(d, [1])
        for n in (1, 33, 130):
            raw = rnd(n, d)
            show("score_dense", "n=%d d=%d" % (n, d), ops.score_dense(ops.score_prepare(raw), d))
            show("backend_plda_dense", "n=%d d=%d" % (n, d), ops.backend_plda_dense(ops.backend_plda_normalize(raw, d, psi), d, *tabs))


def vbx():
    t, d, s, (fa, fb, lp) = 200, 128, 6, vbx_ref.PARAMS[0]
    cases = [vbx_ref.make_case(t, d, s, seed) for seed in range(2)]
    x, gamma = (dev(np.concatenate([c[k].ravel() for c in cases])) for k in ("x", "gamma"))
    pi = dev(np.concatenate([c["pi"] for c in cases]))
    out = ops.vbx(x, np.arange(2, dtype=np.int64) * t * d, np.full(2, t, np.int32), d, dev(cases[0]["phi"].copy()), gamma, pi, np.full(2, s, np.int32),
                  loop_prob=lp, fa=fa, fb=fb, max_iters=5, epsilon=-np.inf)
    show("vbx", "(T, D, S)=(200, 128, 6) x 2, 5 iterations", *out)


def pca_plda():
    for d, n in ((36, 40), (130, 129)):      # the eigenproblems in LDS, and the first one in the workspace
        c = pca_plda_ref.case(d, n)
        xs = [pca_plda_ref.recording(seed, d, n) for seed in range(2)]
        out = ops.backend_pca_plda(dev(np.concatenate([x.ravel() for x in xs])), np.arange(2, dtype=np.int64) * n * d, np.full(2, n, np.int64), d,
                                   dev(np.array(c["w"])), dev(np.array(c["b"])), dev(np.array(c["mu"])), 0.9)
        show("backend_pca_plda", "(n, D)=(%d, %d) x 2, target 0.9" % (n, d), *(out[k] for k in sorted(out)))


if __name__ == "__main__":
    row_ops()
    cohort_ops()
    dense_ops()
    vbx()
    pca_plda()
    torch.cuda.synchronize()
