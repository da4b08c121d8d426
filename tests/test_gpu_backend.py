"""The LDA / PLDA back end on a real MI355X: the ops of csrc/xv_backend.hip through ops.py, Backend.train, BackendScorer and the two drivers
against the fp64 restatement (tests/backend_ref.py), which reads the same fp32 inputs in double.

Tolerances (EPS = 2^-24, chain(d) = 4 * ceil(d / 256) + 6 as stated in csrc/xv_rowsum.h):
  group means        mean64 bit-equal to the sequential fp64 loop (same order, IEEE adds and one IEEE divide; the build has no fast-math
                     flag); mean32 == float32(mean64)
  scatter            2 * (c_blk + 2) * EPS * sum_r |v_ri v_rj| per element, from the fp64 products.  c_blk = the reduction rows one
                     workgroup of the TN GEMM accumulates in fp32: out[2] of xv_debug_tn_plan(d4, d4, block rows) - the plan
                     xv_launch_gemm_tn runs (csrc/xv_gemm_tn.hip, xv_tn_plan: "`chunk` reduction rows per workgroup"), the larger of the
                     full block's and the tail block's.  An accumulator takes chunk / 2 MFMA steps of two products each: at most c_blk
                     roundings; the products are exact in the sum's precision only after one rounding each (+ 1); v itself is reproduced
                     exactly by the reference (an fp32 subtraction); the slabs and blocks are added in double (+ 1 covers it generously).
                     The result is bit-symmetric (an element is read from the upper triangle of the slabs) and the same bits on a second call.
  plda_normalize     2 * (chain(d) + 2) * EPS * sum_c ref_c^2 / (psi_c + 1 / n) of the reference row (= d for every non-zero row), per
                     element - the form of test_gpu_score.py::test_prepare: a term carries three roundings (1 / n, psi + 1 / n, the divide),
                     the sum chain(d), half of that reaches the output, plus sqrt, the divide d / s and the product: below 0.5 chain + 7.
  plda_trials        2 * (2 * chain(d) + 6) * EPS * sum_c (|0.5 iv (t - a e)^2| + |0.5 g t^2|) + EPS * |k0| per trial, from the fp64 terms of
                     the SAME fp32 tables.  The kernel's own first-order worst case is (2 chain(d) - 2) EPS * sum + EPS |k0| (header of
                     csrc/xv_backend.hip: 2 chain - 6 adds, three roundings inside a term, the final k0 + s), inside the asserted bound.
  chain              the GEMM figure (2e-5 of the operand norms) per affine map composed with the row tolerances above
                     (_chain_tol).
  end to end         4 * Delta_ref + the trial tolerance, Delta_ref measured inside the test (see test_end_to_end).
"""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import backend_ref as R

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
GEMM_TOL = 2e-5
BLOCK = 8192
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "tf_kaldi_speaker_amd")
DEV = "cuda:0"


def _ops():
    import torch
    from tf_kaldi_speaker_amd import ops
    return torch, ops


def _pitched(torch, a, ld, fill=1e3, offset=0):
    rows, d = a.shape
    flat = torch.full((rows * ld + offset,), fill, dtype=torch.float32, device=DEV)
    buf = flat[offset:].view(rows, ld)
    if d:
        buf[:, :d] = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)
    return buf


def _c_blk(n, d):
    from tf_kaldi_speaker_amd import _lib
    dp = (d + 3) // 4 * 4
    out = (C.c_int * 4)()
    chunks = []
    for r in sorted({min(n, BLOCK), n % BLOCK or BLOCK} if n > BLOCK else {n}):
        _lib.call("xv_debug_tn_plan", dp, dp, r, 0, out)
        chunks.append(out[2])
    return max(chunks)


# ---- group means ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("groups", [1, 37])
@pytest.mark.parametrize("d", [1, 30, 512, 601])
def test_group_means(d, groups):
    torch, ops = _ops()
    rs = np.random.RandomState(d + groups)
    n = 400
    x = (rs.randn(n, d) * 3 + 0.5).astype(np.float32)
    sizes = [300] if groups == 1 else [(1, 2, 65, 300)[g % 4] for g in range(groups)]
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    rows = rs.randint(0, n, int(offsets[-1]))                  # non-monotone, with repeats across and within groups
    for g, s in enumerate(sizes):
        if s >= 2:
            rows[offsets[g] + 1] = rows[offsets[g]]             # one row twice in a row
    xb = _pitched(torch, x, d + 3, offset=1)                    # pitched, 1e3 in the padding, base off the 16-byte grid
    m64, m32 = ops.backend_group_means(xb, d, offsets, rows)
    want = R.group_means(x, d, offsets, rows)
    got = m64.cpu().numpy()
    assert got.dtype == np.float64 and got.shape == want.shape
    assert np.array_equal(got.view(np.int64), want.view(np.int64)), float(np.abs(got - want).max())
    got32 = m32.cpu().numpy()
    d4 = (d + 3) // 4 * 4
    assert got32.shape == (groups, d4) and np.array_equal(got32[:, :d], want.astype(np.float32)) and np.all(got32[:, d:] == 0.0)
    assert np.all(xb.cpu().numpy()[:, d:] == 1e3)
    only64, none32 = ops.backend_group_means(xb, d, offsets, rows, want32=False)
    assert none32 is None and torch.equal(only64, m64)


# ---- scatter ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scatter_data():
    rs = np.random.RandomState(5)
    return (rs.randn(3 * BLOCK, 200) * 2 + 0.3).astype(np.float32), rs.randn(200).astype(np.float32)


@pytest.mark.parametrize("with_mean", [False, True])
@pytest.mark.parametrize("n,d", [(1, 30), (129, 200), (BLOCK + 129, 64), (3 * BLOCK, 30)])
def test_scatter(scatter_data, n, d, with_mean):
    torch, ops = _ops()
    xs, means = scatter_data
    x = xs[:n, :d]
    mean = means[:d].copy() if with_mean else None
    mean_d = torch.from_numpy(mean).to(DEV) if with_mean else None
    v = R.center(x, mean)
    want, tol = R.scatter(v), 2 * (_c_blk(n, d) + 2) * EPS * R.scatter_abs(v)
    worst = 0.0
    # an operand as it stands when d % 4 == 0 and nothing is subtracted (no copy), then a pitch and base off the 16-byte grid (copied)
    for xb in (torch.from_numpy(np.ascontiguousarray(x)).to(DEV), _pitched(torch, x, d + 3, offset=1)):
        c = ops.backend_scatter(xb, d=d, mean=mean_d)
        got = c.cpu().numpy()
        err = np.abs(got - want)
        assert got.shape == (d, d) and np.all(err <= tol), float((err / np.maximum(tol, 1e-300)).max())
        assert torch.equal(c, c.t())                                              # bit-symmetric, as the header states
        assert torch.equal(c, ops.backend_scatter(xb, d=d, mean=mean_d))          # the same bits on a second call
        worst = max(worst, float((err / np.maximum(tol, 1e-300)).max()))
    print("scatter n=%d d=%d mean=%s c_blk=%d: worst error / bound %.4f" % (n, d, with_mean, _c_blk(n, d), worst))


# ---- plda_normalize ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def norm_data():
    rs = np.random.RandomState(9)
    return (rs.randn(129, 601) * 2).astype(np.float32), rs.uniform(0.05, 4.0, 601).astype(np.float32), rs.choice([1, 3, 8], 129)


@pytest.mark.parametrize("rows", [1, 3, 129])
@pytest.mark.parametrize("d", [1, 30, 200, 512, 601])
def test_plda_normalize(norm_data, d, rows):
    torch, ops = _ops()
    us, psis, ns = norm_data
    u, psi = us[:rows, :d].copy(), psis[:d].copy()
    zero_row = rows // 2 if rows >= 3 else None
    if zero_row is not None:
        u[zero_row] = 0.0
    d4 = (d + 3) // 4 * 4
    worst = 0.0
    for n_utts in (None, ns[:rows]):
        ref = R.plda_normalize(u, psi, n_utts)
        w = 1.0 / (psi.astype(np.float64)[None, :] + 1.0 / (np.ones(rows) if n_utts is None else n_utts.astype(np.float64))[:, None])
        tol = 2 * (R.chain(d) + 2) * EPS * (ref * ref * w).sum(axis=1, keepdims=True)
        for ldu, ldo, off in ((d4 + 4, d4 + 8, 0), (d + 1, d + 3, 1)):
            psi_d = _pitched(torch, psi[None, :], d, offset=off)[0]
            ub = _pitched(torch, u, ldu, offset=off)
            out = _pitched(torch, np.zeros((rows, 0), np.float32), ldo, offset=off)
            got = ops.backend_plda_normalize(ub, d, psi_d, n_utts=n_utts, out=out)
            assert got.data_ptr() == out.data_ptr()
            inplace = ops.backend_plda_normalize(ub, d, psi_d, n_utts=n_utts, out=ub)
            assert inplace.data_ptr() == ub.data_ptr()
            for g in (got.cpu().numpy(), inplace.cpu().numpy()):
                err = np.abs(g[:, :d].astype(np.float64) - ref)
                assert np.all(err <= tol), (d, rows, float((err / np.maximum(tol, 1e-300)).max()))
                assert np.all(g[:, d:] == 0.0)
                if zero_row is not None:
                    assert np.all(g[zero_row] == 0.0) and np.all(ref[zero_row] == 0.0)
                worst = max(worst, float((err / np.maximum(tol, 1e-300)).max()))
    print("plda_normalize d=%d rows=%d: worst error / bound %.3f" % (d, rows, worst))


# ---- plda_trials ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 5, 1025])
@pytest.mark.parametrize("d", [30, 200, 512, 601])
def test_plda_trials(d, m):
    from tf_kaldi_speaker_amd.misc import backend as B
    torch, ops = _ops()
    rs = np.random.RandomState(d)
    psi = np.sort(rs.uniform(0.02, 6.0, d))[::-1].copy()
    n_e = rs.choice([1, 3, 8], 9)
    n_e[:3] = (1, 3, 8)
    distinct, nidx = np.unique(n_e, return_inverse=True)
    coef, g, k0 = B.plda_coefficients(psi, distinct)
    e = (rs.randn(9, d) * np.sqrt(psi + 0.3)).astype(np.float32)
    t = (rs.randn(7, d) * np.sqrt(psi + 1.0)).astype(np.float32)
    t[0] = coef[nidx[0], 0, :d] * e[0]              # target-like: t = a e, the first form about 0
    t[1] = -20.0 * e[1]                             # far: |t - e| large
    ei = (np.arange(m)[::-1] % 9).astype(np.int64)
    ti = rs.randint(0, 7, m)
    ei[0], ti[0] = 0, 0
    if m >= 5:
        ei[1], ti[1] = 1, 1
        ei[2], ti[2] = ei[3], ti[3]                  # one trial twice in a row
    ldc = coef.shape[2]
    want, terms, k0q = R.trials_from_tables(e, t, ei, ti, nidx, coef, g, k0, d)
    tol = 2 * (2 * R.chain(d) + 6) * EPS * terms + EPS * np.abs(k0q)
    coef_d, g_d, k0_d = (torch.from_numpy(a).to(DEV) for a in (coef, g, k0))
    worst = 0.0
    # pitches on the 16-byte grid (the vector path when d % 4 == 0), then pitches off by one (the scalar path)
    for lde, ldt in ((ldc + 4, ldc + 8), (ldc + 1, ldc + 5)):
        eb, tb = _pitched(torch, e, lde), _pitched(torch, t, ldt)
        got = ops.backend_plda_trials(eb, tb, d, ei, ti, nidx, coef_d, g_d, k0_d).cpu().numpy().astype(np.float64)
        err = np.abs(got - want)
        assert got.shape == (m,) and np.all(err <= tol), float((err / tol).max())
        worst = max(worst, float((err / tol).max()))
    # the tables are the restatement's closed form: target-like trial 0 scores far above the far trial
    full = R.llr_trials(e, t, ei, ti, psi, n_e)
    assert np.all(np.abs(full - want) <= 1e-5 * (terms + np.abs(k0q)))
    print("plda_trials d=%d m=%d: worst error / bound %.3f (target-like %.3f, far %.3g)" % (d, m, worst, want[0], want[1] if m >= 5 else np.nan))


# ---- the chain --------------------------------------------------------------------------------------------------------------------------
def _chain_tol(be, x, n_utts, plda):
    """Per-element bound of the prepared tables: each affine map at the GEMM figure (2e-5 of |operand row| * |weight row|, + the bias),
    the unit normalisation at score_prepare's row tolerance, the PLDA normalisation at plda_normalize's; first-order propagation."""
    v = R.center(x, be.mean)
    if be.lda is not None:
        a = be.lda.astype(np.float64)
        z = R.transform_vec(a, v)
        dz = GEMM_TOL * (np.linalg.norm(v, axis=1, keepdims=True) * np.linalg.norm(a[:, :-1], axis=1)[None, :] + np.abs(a[:, -1])[None, :])
    else:
        z, dz = v, np.zeros_like(v)
    dim = z.shape[1]
    p = 2 * (R.chain(dim) + 2) * EPS
    dy = 2 * np.linalg.norm(dz, axis=1, keepdims=True) / np.linalg.norm(z, axis=1, keepdims=True) + p      # 2-norm bound of a unit row's error
    if not plda:
        return dy * np.ones((1, dim))
    w = np.sqrt(float(dim)) * be.plda["transform"]
    b = -(be.plda["transform"] @ be.plda["mean"])
    wn = np.linalg.norm(w, axis=1)[None, :]
    y = z / np.linalg.norm(z, axis=1, keepdims=True)
    u = y @ w.T + b
    du = wn * dy + GEMM_TOL * (wn + np.abs(b)[None, :])
    wt = 1.0 / (be.plda["psi"][None, :] + 1.0 / (np.ones(len(x)) if n_utts is None else np.asarray(n_utts, dtype=np.float64))[:, None])
    s2 = (u * u * wt).sum(axis=1, keepdims=True)
    scale = np.sqrt(dim / s2)
    rel_s = np.sqrt((du * du * wt).sum(axis=1, keepdims=True) / s2)
    return scale * du + np.abs(u) * scale * rel_s + 2 * (R.chain(dim) + 2) * EPS * dim


def _synthetic_backend(rs, d, dim):
    from tf_kaldi_speaker_amd.misc import backend as B
    q, _ = np.linalg.qr(rs.randn(dim, dim))
    plda = dict(mean=rs.randn(dim) * 0.2, transform=q * rs.uniform(0.5, 2.0, dim)[:, None], psi=np.sort(rs.uniform(0.05, 5.0, dim))[::-1].copy())
    return B.Backend((rs.randn(d) * 0.3).astype(np.float32), (rs.randn(dim, d + 1) / 8).astype(np.float32), plda)


def test_chain_matches_the_restatement():
    from tf_kaldi_speaker_amd.misc import backend as B
    rs = np.random.RandomState(21)
    d, dim, rows = 64, 16, 300
    be = _synthetic_backend(rs, d, dim)
    x = (rs.randn(rows, d) + 0.3).astype(np.float32)
    n_utts = rs.choice([1, 3, 8], rows)
    model = dict(be.plda, offset=-(be.plda["transform"] @ be.plda["mean"]))
    unit = R.unit_chain(be.mean, be.lda, x)
    got = B.BackendScorer(be, "lda_cos", DEV).prepare(x).cpu().numpy()
    tol = _chain_tol(be, x, None, False)
    assert got.shape == (rows, dim) and np.all(np.abs(got - unit) <= tol), float((np.abs(got - unit) / tol).max())
    sc = B.BackendScorer(be, "plda", DEV)
    for n in (None, n_utts):
        want = R.plda_transform(model, unit * np.sqrt(float(dim)), n)
        got = sc.prepare(x, n_utts=n).cpu().numpy()
        tol = _chain_tol(be, x, n, True)
        assert got.shape == (rows, dim) and np.all(np.abs(got - want) <= tol), float((np.abs(got - want) / tol).max())
        print("chain n_utts=%s: worst error / bound %.4f" % (n is not None, float((np.abs(got - want) / tol).max())))


# ---- end to end -------------------------------------------------------------------------------------------------------------------------
def planted(seed, speakers, d, rank, max_n, spread=1.0):
    """Planted data: speaker means in a rank-`rank` subspace, unit within-class noise, a global offset.  -> (x fp32, groups)."""
    rs = np.random.RandomState(seed)
    basis = np.linalg.qr(rs.randn(d, d))[0][:, :rank] * (spread * np.linspace(3.0, 1.5, rank))[None, :]
    counts = rs.randint(1, max_n + 1, speakers)
    groups, rows, at = [], [], 0
    for n in counts:
        m = basis @ rs.randn(rank)
        rows.append(m[None, :] + rs.randn(n, d))
        groups.append(list(range(at, at + n)))
        at += n
    return (np.concatenate(rows) + rs.randn(d) * 0.5).astype(np.float32), groups


def _trials(rs, groups, m, target_share=0.2):
    spk_of = np.concatenate([[s] * len(g) for s, g in enumerate(groups)])
    ei, ti = [], []
    while len(ei) < m:
        a = rs.randint(0, len(spk_of))
        if len(ei) < target_share * m:
            b = rs.choice(groups[spk_of[a]])
            if a == b:
                continue
        else:
            b = rs.randint(0, len(spk_of))
            if spk_of[a] == spk_of[b]:
                continue
        ei.append(a)
        ti.append(b)
    ei, ti = np.asarray(ei), np.asarray(ti)
    return ei, ti, spk_of[ei] == spk_of[ti]


def test_end_to_end_train_and_score():
    """Backend.train on the GPU against the restatement trained on exact fp64 statistics.  The bound is measured, not fixed: the restatement
    is retrained on its own two scatter statistics perturbed entrywise by +- the scatter tolerance (random signs, symmetrised; three seeds);
    Delta_ref = the largest score movement; the GPU-trained model's scores must lie within 4 * Delta_ref + the trial tolerance (random signs are not the
    worst case).  profiles/backend_e2e_sensitivity.txt records the run: Delta_ref 1.115e-02, observed maximum 3.5e-05, both EERs 1.75 %."""
    from tf_kaldi_speaker_amd.misc import backend as B
    d, dim = 64, 16
    x, groups = planted(3, 300, d, 12, 9)
    keys = ["u%05d" % i for i in range(len(x))]
    spk2utt = [("s%03d" % s, [keys[i] for i in g]) for s, g in enumerate(groups)]
    ei, ti, targets = _trials(np.random.RandomState(4), groups, 2000)
    mean, lda_mat, plda = R.train(x, groups, dim)
    want = R.score(mean, lda_mat, plda, x, x, ei, ti, "plda")
    eer_ref = R.eer(want, targets)
    assert eer_ref < 0.10, eer_ref                                # the data is not degenerate (asserted on the reference alone)
    c_blk = _c_blk(len(x), d)

    def perturbed(seed):
        rs = np.random.RandomState(seed)
        def perturb(name, stat, abs_stat):
            tol = 2 * (c_blk + 2) * EPS * abs_stat                   # tol_ij of test_scatter
            sgn = np.triu(rs.choice([-1.0, 1.0], stat.shape))
            return stat + tol * (sgn + np.triu(sgn, 1).T)
        m2, l2, p2 = R.train(x, groups, dim, perturb=perturb)
        return R.score(m2, l2, p2, x, x, ei, ti, "plda")

    delta_ref = max(float(np.abs(perturbed(s) - want).max()) for s in (11, 12, 13))
    be = B.Backend.train(x, keys, spk2utt, lda_dim=dim, device=DEV)
    sc = B.BackendScorer(be, "plda", DEV)
    prep = sc.prepare(x)
    got = sc.score(prep, prep, ei, ti).astype(np.float64)
    # the trial tolerance from the reference's own terms
    e_u = R.plda_transform(plda, R.unit_chain(mean, lda_mat, x) * np.sqrt(float(dim)))
    a, iv, g, k0 = R.coefficients(plda["psi"], [1])
    terms = (np.abs(0.5 * iv[0] * (e_u[ti] - a[0] * e_u[ei]) ** 2) + np.abs(0.5 * g * e_u[ti] ** 2)).sum(axis=1)
    tol = 4 * delta_ref + 2 * (2 * R.chain(dim) + 6) * EPS * terms + EPS * abs(k0[0])
    err = np.abs(got - want)
    eer_gpu = R.eer(got, targets)
    print("end to end: Delta_ref %.3e, observed max |score difference| %.3e, bound min %.3e; EER reference %.3f%%, GPU %.3f%%"
          % (delta_ref, float(err.max()), float(tol.min()), 100 * eer_ref, 100 * eer_gpu))
    assert np.all(err <= tol), float((err / tol).max())
    assert abs(eer_gpu - eer_ref) <= 0.01


# ---- the drivers ------------------------------------------------------------------------------------------------------------------------
def _write_table(path, keys, matrix):
    from tf_kaldi_speaker_amd.dataset import kaldi_io
    with open(path + ".ark", "wb") as f:
        for k, v in zip(keys, matrix):
            kaldi_io.write_vec_flt(f, v, key=k)
    return "ark:%s.ark" % path


def _run(script, args, cwd):
    env = dict(os.environ, TF_KALDI_ROOT=PKG, PYTHONPATH=PKG)
    return subprocess.run([sys.executable, os.path.join(PKG, "nnet", "lib", script)] + args, env=env, cwd=cwd, capture_output=True, text=True, timeout=300)


def test_drivers(tmp_path):
    """train_backend.py, then score.py --backend --scoring plda --enrol-spk2utt, --scoring lda_cos, and score.py without a new option, each a
    fresh child process under its own timeout."""
    from tf_kaldi_speaker_amd.misc import backend as B
    from tf_kaldi_speaker_amd.misc import scoring
    d, dim = 24, 8
    x, groups = planted(8, 40, d, 6, 6)
    keys = ["u%04d" % i for i in range(len(x))]
    spk = ["s%02d" % s for s in range(len(groups))]
    train_spec = _write_table(str(tmp_path / "train"), keys, x)
    with open(tmp_path / "spk2utt", "w") as f:
        f.write("".join("%s %s\n" % (spk[s], " ".join(keys[i] for i in g)) for s, g in enumerate(groups)))
        f.write("ghost u9998 u9999\n")                                         # a speaker without any vector: dropped
    bdir = str(tmp_path / "backend")
    r = _run("train_backend.py", ["--lda-dim", str(dim), train_spec, str(tmp_path / "spk2utt"), bdir], str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    assert "N = %d vectors of K = 40 speakers" % len(x) in r.stderr and "Speaker ghost: no vector for any utterance, dropped." in r.stderr
    assert re.search(r"LDA: kept eigenvalues \S+ \.\. \S+", r.stderr) and re.search(r"PLDA: psi min \S+, max \S+", r.stderr)
    assert sorted(os.listdir(bdir)) == ["mean.vec", "plda", "transform.mat"]
    be = B.Backend.load(bdir)
    model = dict(be.plda, offset=-(be.plda["transform"] @ be.plda["mean"]))
    # enrolment: fresh utterances of the first 20 speakers, 1 .. 4 each; one listed utterance has no vector (skipped)
    ex, eg = x, groups                                                         # (plumbing: the training rows serve as enrolment and test utterances)
    e_groups = [g[:max(1, len(g) // 2)] for g in eg[:20]]
    t_rows = [g[-1] for g in eg[:20] if len(g) >= 2]
    t_spk = [s for s, g in enumerate(eg[:20]) if len(g) >= 2]
    e_rows = sorted(i for g in e_groups for i in g)
    e_spec = _write_table(str(tmp_path / "enrol"), [keys[i] for i in e_rows], ex[e_rows])
    t_spec = _write_table(str(tmp_path / "test"), ["t%02d" % s for s in t_spk], ex[t_rows])
    with open(tmp_path / "enrol_spk2utt", "w") as f:
        f.write("".join("%s %s%s\n" % (spk[s], " ".join(keys[i] for i in g), " u9999" if s == 0 else "") for s, g in enumerate(e_groups)))
    listed = [(spk[a], "t%02d" % b, a == b) for a in range(20) for b in t_spk[:6]]
    listed.insert(5, ("s39", "t00", False))                                    # a speaker that was not enrolled: skipped
    with open(tmp_path / "trials", "w") as f:
        f.write("".join("%s %s %s\n" % (a, b, "target" if lab else "nontarget") for a, b, lab in listed))
    kept = [tr for tr in listed if tr[0] != "s39"]
    ei = np.asarray([spk.index(a) for a, _, _ in kept])
    ti = np.asarray([t_spk.index(int(b[1:])) for _, b, _ in kept])
    counts = np.asarray([len(g) for g in e_groups])
    offsets = np.concatenate([[0], np.cumsum(counts)])
    rows = np.concatenate([[e_rows.index(i) for i in g] for g in e_groups])
    avg = R.group_means(ex[e_rows], d, offsets, rows).astype(np.float32)       # fp64 accumulation, rounded once
    test = ex[t_rows]
    out = str(tmp_path / "scores")
    for mode in ("plda", "lda_cos"):
        r = _run("score.py", ["--backend", bdir, "--scoring", mode, "--enrol-spk2utt", str(tmp_path / "enrol_spk2utt"), str(tmp_path / "trials"),
                              e_spec, t_spec, out], str(tmp_path))
        assert r.returncode == 0, r.stderr[-2000:]
        lines = open(out).read().splitlines()
        assert [ln.split()[:2] for ln in lines] == [[a, b] for a, b, _ in kept]
        got = np.array([float(ln.split()[2]) for ln in lines])
        assert "Trial s39 t00: no vector for a key, skip." in r.stderr and "Scored %d trials, skipped 1." % len(kept) in r.stderr
        assert "Utterance u9999 of speaker s00: no vector, skip." in r.stderr
        assert re.search(r"EER ([0-9.]+)%  minDCF08 ([0-9.]+)  minDCF10 ([0-9.]+)", r.stderr)
        want = R.score(be.mean, be.lda, model, avg, test, ei, ti, mode, enrol_n=counts)
        te, tt = _chain_tol(be, avg, counts, mode == "plda"), _chain_tol(be, test, None, mode == "plda")
        if mode == "lda_cos":
            tol = te[ei, 0] + tt[ti, 0] + 2 * (R.chain(dim) + 2) * EPS      # (a unit row's bound is a 2-norm bound, the same in every column)
        else:
            # first-order propagation of the prepared rows' bounds through the log-likelihood ratio, plus the trial tolerance
            eu = R.plda_transform(model, R.unit_chain(be.mean, be.lda, avg) * np.sqrt(float(dim)), counts)
            tu = R.plda_transform(model, R.unit_chain(be.mean, be.lda, test) * np.sqrt(float(dim)))
            n = counts[ei].astype(np.float64)[:, None]
            psi = be.plda["psi"][None, :]
            a, v = n * psi / (n * psi + 1), 1 + psi / (n * psi + 1)
            diff = tu[ti] - a * eu[ei]
            grad = (np.abs(diff / v) * (tt[ti] + a * te[ei]) + np.abs(tu[ti] / (psi + 1)) * tt[ti]).sum(axis=1)
            terms = (np.abs(0.5 * diff ** 2 / v) + np.abs(0.5 * tu[ti] ** 2 / (psi + 1))).sum(axis=1)
            tol = grad + 2 * (2 * R.chain(dim) + 6) * EPS * terms + 4 * EPS * np.abs(want)
        assert np.all(np.abs(got - want) <= tol + 5e-7), (mode, float((np.abs(got - want) / (tol + 5e-7)).max()))
    # no new option: the bytes CosineScorer's scores print as
    with open(tmp_path / "trials_c", "w") as f:
        f.write("".join("%s %s\n" % (keys[e_rows[a]], "t%02d" % b) for a in range(10) for b in t_spk[:5]))
    r = _run("score.py", [str(tmp_path / "trials_c"), e_spec, t_spec, out], str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    csc = scoring.CosineScorer(DEV)
    ci, cj = np.repeat(np.arange(10), 5), np.tile(np.arange(5), 10)
    direct = csc.score(csc.prepare(ex[e_rows]), csc.prepare(test), ci, cj)
    assert open(out).read() == "".join("%s %s %.6f\n" % (keys[e_rows[a]], "t%02d" % t_spk[b], s) for a, b, s in zip(ci, cj, direct))


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_are_returned():
    from tf_kaldi_speaker_amd._lib import XvError
    from tf_kaldi_speaker_amd.misc import backend as B
    torch, ops = _ops()
    x = torch.ones((16, 8), dtype=torch.float32, device=DEV)
    psi = torch.ones(8, dtype=torch.float32, device=DEV)
    with pytest.raises(ValueError, match="group 1 is empty"):
        ops.backend_group_means(x, 8, [0, 2, 2, 3], [0, 1, 2])
    with pytest.raises(IndexError, match="rows holds a value outside"):
        ops.backend_group_means(x, 8, [0, 2], [0, 16])
    with pytest.raises(XvError, match="workspace of 64 bytes"):
        ops.backend_scatter(x, ws_bytes=64)                     # less than one 8 x 8 slab
    with pytest.raises(XvError, match="u and out overlap"):
        ops.backend_plda_normalize(x[:15], 8, psi, out=x[1:])
    with pytest.raises(XvError, match="x and y overlap"):
        ops.backend_center(x[:15], out=x[1:])
    for call in (lambda: ops.backend_scatter(x, d=0), lambda: ops.backend_group_means(x, 0, [0, 1], [0]),
                 lambda: ops.backend_plda_normalize(x, 0, psi[:0])):
        with pytest.raises(XvError, match="d must be positive"):
            call()
    coef, g, k0 = (torch.from_numpy(a).to(DEV) for a in B.plda_coefficients(np.ones(8), [1, 3]))
    with pytest.raises(IndexError, match="nidx holds a value outside 0 .. 1"):
        ops.backend_plda_trials(x, x, 8, [0], [1], [2] + [0] * 15, coef, g, k0)
    with pytest.raises(IndexError, match="ei holds a value outside"):
        ops.backend_plda_trials(x, x, 8, [16], [1], [0] * 16, coef, g, k0)
    got = ops.backend_plda_trials(x, x, 8, [0], [1], [1] + [0] * 15, coef, g, k0)      # and the device still works afterwards
    assert got.shape == (1,) and np.isfinite(got.cpu().numpy()).all()
