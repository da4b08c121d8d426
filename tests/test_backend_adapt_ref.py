"""CPU checks of PLDA domain adaptation and of the dense / AS-normed PLDA scores: the fp64 restatement (tests/backend_adapt_ref.py) against
derivations that do not share its code, misc.backend.adapt_plda against the restatement, the `plda` file round trip of an adapted model, and
the refusals of nnet/lib/adapt_backend.py and nnet/lib/score.py --scoring plda_asnorm, which come before the GPU is touched."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import backend_adapt_ref as A
from tests import backend_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "tf_kaldi_speaker_amd")


def _model(rs, d):
    q, _ = np.linalg.qr(rs.randn(d, d))
    return dict(mean=rs.randn(d) * 0.3, transform=(q * rs.uniform(0.5, 2.0, d)[:, None]) @ np.linalg.qr(rs.randn(d, d))[0],
                psi=np.sort(rs.uniform(0.05, 5.0, d))[::-1].copy())


def _in_domain(rs, model, n, scale_dirs=4, factor=2.5, shrink=1.0, offset=0.4):
    """Samples whose covariance is the model's total covariance rotated, a few directions scaled by `factor`, all by `shrink`, and offset."""
    d = model["psi"].shape[0]
    c = np.linalg.cholesky(A.total_covariance(model))
    rot = np.linalg.qr(rs.randn(d, d))[0]
    gains = np.full(d, shrink)
    gains[:scale_dirs] *= factor
    return (rs.randn(n, d) * gains) @ rot.T @ c.T + model["mean"] + offset * rs.randn(d)


def test_llr_factorisation_and_symmetry():
    """LLR(e, t) = R(e) + C_q(t) + sum_c (iv a e_c) t_c against the closed form of backend_ref.llr_trials, and LLR symmetric for n = 1."""
    rs = np.random.RandomState(0)
    d = 30
    psi = np.sort(rs.uniform(0.02, 6.0, d))[::-1]
    counts = np.array([1, 3, 8])
    n_e = counts[rs.randint(0, 3, 11)]
    e, t = rs.randn(11, d) * np.sqrt(psi + 0.3), rs.randn(7, d) * np.sqrt(psi + 1.0)
    a, iv, g, k0 = R.coefficients(psi, counts)
    q = np.searchsorted(counts, n_e)
    r_term = k0[q] - 0.5 * (iv[q] * a[q] ** 2 * e * e).sum(axis=1)
    c_term = 0.5 * ((g[None, :] - iv)[:, None, :] * (t * t)[None, :, :]).sum(axis=2)            # [q, j]
    dense = (iv[q] * a[q] * e) @ t.T + c_term[q] + r_term[:, None]
    want = A.dense_llr(e, t, psi, n_e)
    assert np.abs(dense - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    sym = A.dense_llr(e, t, psi)
    assert np.abs(sym - A.dense_llr(t, e, psi).T).max() <= 1e-12 * max(1.0, np.abs(sym).max())


def test_as_norm_against_a_literal_loop():
    rs = np.random.RandomState(1)
    d = 6
    psi = np.sort(rs.uniform(0.1, 3.0, d))[::-1]
    e, t, c = rs.randn(3, d), rs.randn(4, d), rs.randn(9, d)
    n_e = np.array([1, 4, 2])
    ei, ti = np.array([0, 1, 2, 1]), np.array([3, 0, 1, 1])
    got, raw, e_stats, t_stats = A.as_norm(e, t, c, ei, ti, psi, 4, n_e)
    for j in range(4):
        s = R.llr(e[ei[j]], t[ti[j]], psi, float(n_e[ei[j]]))
        se = sorted((R.llr(e[ei[j]], cj, psi, float(n_e[ei[j]])) for cj in c), reverse=True)[:4]
        st = sorted((R.llr(t[ti[j]], cj, psi, 1.0) for cj in c), reverse=True)[:4]
        want = 0.5 * ((s - np.mean(se)) / np.std(se) + (s - np.mean(st)) / np.std(st))
        assert abs(raw[j] - s) <= 1e-12 * max(1.0, abs(s)) and abs(got[j] - want) <= 1e-10 * max(1.0, abs(want))
    assert np.all(A.top_k_stats(np.full((2, 5), 0.25), 3)[:, 1] == 1e-6)                        # the floor


def test_total_covariance_identity_when_the_scales_sum_to_one():
    """within + between = 1: the adapted model's total covariance is M^-1 P diag(max(s, 1)) P^T M^-T."""
    rs = np.random.RandomState(2)
    d = 24
    model = _model(rs, d)
    m, s_y, n = A.adapt_stats(_in_domain(rs, model, 4000))
    for within in (0.75, 0.3, 1.0):
        out = A.adapt(model, m, s_y, n, within, 1.0 - within, 1.0)
        assert 0 < (out["s"] > 1.0).sum() < d                                                   # both branches of step 3 are taken
        v = s_y / n - np.outer(m, m) + np.outer(m - model["mean"], m - model["mean"])
        mm = model["transform"] / np.sqrt(1.0 + model["psi"])[:, None]
        s, p = np.linalg.eigh(mm @ v @ mm.T)
        mi = np.linalg.inv(mm)
        want = mi @ p @ np.diag(np.maximum(s, 1.0)) @ p.T @ mi.T
        got = A.total_covariance(out)
        assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max()


def test_model_comes_back_when_no_eigenvalue_exceeds_one():
    rs = np.random.RandomState(3)
    d = 24
    model = _model(rs, d)
    y = _in_domain(rs, model, 4000, scale_dirs=0, shrink=0.6, offset=0.0)
    m, s_y, n = A.adapt_stats(y)
    out = A.adapt(model, m, s_y, n, 0.75, 0.25, 1.0)
    assert out["s"].max() < 1.0
    assert np.abs(out["psi"] - model["psi"]).max() <= 1e-9 * model["psi"].max()
    assert np.abs(np.abs(out["transform"]) - np.abs(model["transform"])).max() <= 1e-9 * np.abs(model["transform"]).max()
    assert np.array_equal(out["mean"], m)                                                       # the mean is the adaptation set's all the same


def _same_model(got, want, tol=1e-9):
    assert np.abs(got["psi"] - want["psi"]).max() <= tol * max(want["psi"].max(), 1.0)
    gi, wi = np.linalg.inv(got["transform"]), np.linalg.inv(want["transform"])
    for dg, dw in ((1.0, 1.0), (got["psi"], want["psi"])):                                      # within, then between: eigenvector signs are free
        a, b = (gi * dg) @ gi.T, (wi * dw) @ wi.T
        assert np.abs(a - b).max() <= tol * np.abs(b).max()
    assert np.abs(got["mean"] - want["mean"]).max() <= 1e-12


@pytest.mark.parametrize("scales", [(0.3, 0.7, 1.0), (0.75, 0.25, 1.0), (0.75, 0.25, 0.0), (0.0, 0.4, 2.0)])
def test_adapt_plda_against_the_restatement(scales):
    from tf_kaldi_speaker_amd.misc import backend as B
    rs = np.random.RandomState(4)
    d = 24
    model = _model(rs, d)
    m, s_y, n = A.adapt_stats(_in_domain(rs, model, 3000))
    got = B.adapt_plda(model, m, s_y, n, *scales)
    want = A.adapt(model, m, s_y, n, *scales)
    _same_model(got, want)
    assert np.abs(got["eigenvalues"] - want["s"]).max() <= 1e-9 * want["s"].max()
    assert np.abs(got["offset"] + got["transform"] @ m).max() <= 1e-12
    with pytest.raises(ValueError, match="must not be negative"):
        B.adapt_plda(model, m, s_y, n, -0.1, 0.5)
    with pytest.raises(ValueError, match="share one dimension"):
        B.adapt_plda(model, m[:5], s_y, n)


def test_mean_diff_scale_adds_exactly_the_rank_one_term():
    """Every eigenvalue above 1 and within + between = 1: the adapted total covariance is V itself, so mean_diff_scale 1 against 0 differ by
    (m - mean)(m - mean)^T."""
    from tf_kaldi_speaker_amd.misc import backend as B
    rs = np.random.RandomState(5)
    d = 24
    model = _model(rs, d)
    m, s_y, n = A.adapt_stats(_in_domain(rs, model, 3000, scale_dirs=d, factor=3.0, offset=0.8))
    with_diff, without = B.adapt_plda(model, m, s_y, n, 0.6, 0.4, 1.0), B.adapt_plda(model, m, s_y, n, 0.6, 0.4, 0.0)
    assert with_diff["eigenvalues"].min() > 1.0 and without["eigenvalues"].min() > 1.0
    diff = A.total_covariance(with_diff) - A.total_covariance(without)
    want = np.outer(m - model["mean"], m - model["mean"])
    assert np.abs(want).max() > 0.1 and np.abs(diff - want).max() <= 1e-9 * np.abs(A.total_covariance(with_diff)).max()


def test_adapted_model_round_trips_through_the_plda_file(tmp_path):
    from tf_kaldi_speaker_amd.dataset import kaldi_io
    from tf_kaldi_speaker_amd.misc import backend as B
    rs = np.random.RandomState(6)
    model = _model(rs, 12)
    m, s_y, n = A.adapt_stats(_in_domain(rs, model, 500))
    out = B.adapt_plda(model, m, s_y, n, 0.75, 0.25)
    path = str(tmp_path / "plda")
    kaldi_io.write_plda(path, out["mean"], out["transform"], out["psi"])
    mean, transform, psi = kaldi_io.read_plda(path)
    assert np.array_equal(mean, out["mean"]) and np.array_equal(transform, out["transform"]) and np.array_equal(psi, out["psi"])
    be = B.Backend(np.zeros(12, np.float32), None, out)
    be.save(str(tmp_path / "dir"))
    back = B.Backend.load(str(tmp_path / "dir"))
    assert np.array_equal(back.plda["transform"], out["transform"]) and back.lda is None
    moved = back.recentred(np.ones((3, 12), np.float32) * np.arange(3, dtype=np.float32)[:, None])
    assert np.array_equal(moved.mean, np.ones(12, np.float32)) and all(np.array_equal(moved.plda[k], back.plda[k]) for k in back.plda)
    with pytest.raises(ValueError, match="dimension mismatch"):
        back.recentred(np.ones((3, 5), np.float32))


# ---- the drivers' refusals --------------------------------------------------------------------------------------------------------------
def _run(script, args, cwd=None):
    env = dict(os.environ, TF_KALDI_ROOT=PKG, PYTHONPATH=PKG)
    return subprocess.run([sys.executable, os.path.join(PKG, "nnet", "lib", script)] + args, env=env, cwd=cwd, capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("args,what", [
    (["--scoring", "plda_asnorm", "--cohort", "ark:c.ark"], "--scoring plda_asnorm needs --backend DIR"),
    (["--backend", "dir", "--scoring", "plda_asnorm"], "--scoring plda_asnorm needs --cohort RSPECIFIER"),
    (["--backend", "dir", "--scoring", "plda_asnorm", "--cohort", "ark:c.ark", "--top-k", "0"], "--top-k must be positive"),
    (["--backend", "dir", "--scoring", "plda", "--cohort", "ark:c.ark"], "--cohort with --scoring plda is not supported: plda writes raw log-likelihood "
                                                                         "ratios; --scoring plda_asnorm normalises them"),
])
def test_score_cli_refusals_by_name(args, what):
    """Refused before any file is opened or the GPU is touched (the files named here do not exist)."""
    r = _run("score.py", args + ["trials", "ark:e.ark", "ark:t.ark", "out"])
    assert r.returncode != 0 and what in r.stderr, r.stderr[-500:]


def test_adapt_cli_refusals_by_name(tmp_path):
    from tf_kaldi_speaker_amd.dataset import kaldi_io
    from tf_kaldi_speaker_amd.misc import backend as B
    lda_only = str(tmp_path / "lda_only")
    B.Backend(np.zeros(6, np.float32), np.ones((3, 7), np.float32) / 4, None).save(lda_only)
    full = str(tmp_path / "full")
    B.Backend(np.zeros(6, np.float32), None, dict(mean=np.zeros(6), transform=np.eye(6), psi=np.linspace(2, 1, 6))).save(full)
    with open(tmp_path / "x5.ark", "wb") as f:
        kaldi_io.write_vec_flt(f, np.ones(5, np.float32), key="u0")
    with open(tmp_path / "x6.ark", "wb") as f:
        for i in range(3):
            kaldi_io.write_vec_flt(f, np.full(6, float(i), np.float32), key="u%d" % i)
    os.symlink(full, str(tmp_path / "link"))
    x5, x6, out = "ark:%s" % (tmp_path / "x5.ark"), "ark:%s" % (tmp_path / "x6.ark"), str(tmp_path / "out")
    for args, what in (([lda_only, x6, out], "holds no plda file: nothing to adapt"),
                       ([full, x5, out], "dimension mismatch: adapt_rspecifier holds vectors of 5 dimensions"),
                       (["--mean-only", "true", full, x5, out], "dimension mismatch: adapt_rspecifier holds vectors of 5 dimensions"),
                       (["--within-covar-scale", "-0.5", full, x6, out], "--within-covar-scale must not be negative"),
                       (["--between-covar-scale", "-1", full, x6, out], "--between-covar-scale must not be negative"),
                       (["--mean-diff-scale", "-1", full, x6, out], "--mean-diff-scale must not be negative"),
                       ([full, x6, full + "/"], "backend_out == backend_in"),
                       ([full, x6, str(tmp_path / "link")], "backend_out == backend_in"),      # a link to backend_in
                       ([str(tmp_path / "nothing"), x6, out], "no mean.vec: not a back-end directory")):
        r = _run("adapt_backend.py", args)
        assert r.returncode != 0 and what in r.stderr, (args, r.stderr[-500:])
        assert not os.path.exists(out)
    # --mean-only true needs neither a plda file nor the GPU: mean.vec replaced, transform.mat copied
    r = _run("adapt_backend.py", ["--mean-only", "true", lda_only, x6, out])
    assert r.returncode == 0, r.stderr[-1000:]
    assert sorted(os.listdir(out)) == ["mean.vec", "transform.mat"]
    moved = B.Backend.load(out)
    assert np.array_equal(moved.mean, np.ones(6, np.float32)) and np.array_equal(moved.lda, B.Backend.load(lda_only).lda)
