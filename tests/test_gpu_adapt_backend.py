"""PLDA domain adaptation and AS-norm of PLDA scores end to end on a real MI355X: Backend.adapt, BackendScorer.cohort and the drivers
(train_backend.py, adapt_backend.py, score.py --scoring plda / plda_asnorm) against the fp64 restatement (tests/backend_adapt_ref.py).

Tolerances (EPS = 2^-24):
  adaptation     the method of test_gpu_backend.py::test_end_to_end_train_and_score.  The restatement adapts the SAME out-of-domain back end on
                 exact fp64 statistics; it is run again on its scatter statistic perturbed entrywise by +- the scatter tolerance
                 2 (c_blk + 2) EPS sum_r |y_ri y_rj| (random signs, symmetrised; three seeds).  Delta_ref = the largest score movement; the
                 GPU-adapted model's scores must lie within MARGIN * Delta_ref + the trial kernel's own bound 2 (2 chain(dim) + 6) EPS sum |terms|
                 + the final rounding, exactly as that test asserts it (random signs are not the worst case; the margin is that test's 4) -
                 nothing for the transform chain, which the allowance has to cover as it does there.  Wherever the ADAPTED model is scored
                 (Backend.adapt, the drivers' adapted directory) this is the allowance.  profiles/backend_adapt_sensitivity.txt records
                 Delta_ref and the observed difference.
  scoring        a model that is the restatement's bit for bit (the recentred directory, BackendScorer.cohort on it) has no sensitivity
                 allowance; there the prepared rows' bounds (test_gpu_backend.py::_chain_tol) are propagated to first order through the
                 log-likelihood ratio, plus the trial kernel's own bound - the plda branch of test_gpu_backend.py::test_drivers.
  AS-norm        per side (raw + delta) / sigma + |s - mu| 2 delta / sigma^2, halved and added, as test_gpu_score.py::_pipeline_tol propagates
                 it: raw the tolerance of the trial as above, delta the largest bound of the row's cohort scores (the same allowance or
                 propagation with the cohort row in the test role, plus the cohort kernel's own bound c1 EPS sum |terms| stated in
                 csrc/xv_backend_cohort.hip).  BackendScorer.cohort is held a second time to the kernels' bounds alone (_from_prepared)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import backend_adapt_ref as A
from tests import backend_ref as R
from tests.test_gpu_backend import _chain_tol

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
MARGIN = 4.0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "tf_kaldi_speaker_amd")
DEV = "cuda:0"
D, DIM = 48, 24


def planted(seed, speakers, d, rank, max_n, rot=None, gains=None, offset=None):
    """Planted data: speaker means in a rank-`rank` subspace, unit within-class noise; then (the in-domain set) every vector rotated by
    `rot`, scaled per direction by `gains` and moved by `offset`.  -> (x fp32, groups)."""
    rs = np.random.RandomState(seed)
    basis = np.linalg.qr(rs.randn(d, d))[0][:, :rank] * np.linspace(3.0, 1.5, rank)[None, :]
    counts = rs.randint(1, max_n + 1, speakers)
    rows, groups, at = [], [], 0
    for n in counts:
        rows.append((basis @ rs.randn(rank))[None, :] + rs.randn(n, d))
        groups.append(list(range(at, at + n)))
        at += n
    x = np.concatenate(rows)
    if rot is not None:
        x = (x * gains[None, :]) @ rot.T + offset[None, :]
    return x.astype(np.float32), groups


def _c_blk(n, d):
    from tf_kaldi_speaker_amd import _lib
    dp = (d + 3) // 4 * 4
    out = (C.c_int * 4)()
    _lib.call("xv_debug_tn_plan", dp, dp, min(n, 8192), 0, out)
    return out[2]


@pytest.fixture(scope="module")
def world():
    """The out-of-domain training set (basis seed 1), the back end trained on it ON THE GPU (both sides adapt this one), and an in-domain
    world from the same speaker subspace (same seed, so the same basis), rotated, 6 directions scaled by 2.5 and offset: an adaptation
    table, and enrolment / test / cohort utterances of further speakers."""
    from tf_kaldi_speaker_amd.misc import backend as B
    x_out, groups = planted(1, 200, D, 20, 6)
    keys = ["o%05d" % i for i in range(len(x_out))]
    spk2utt = [("s%03d" % s, [keys[i] for i in g]) for s, g in enumerate(groups)]
    be = B.Backend.train(x_out, keys, spk2utt, lda_dim=DIM, device=DEV)
    rs = np.random.RandomState(2)
    rot = np.linalg.qr(rs.randn(D, D))[0]
    rot = np.linalg.qr(np.eye(D) + 0.25 * (rot - rot.T))[0]                       # a moderate rotation
    gains = np.ones(D)
    gains[:6] = 2.5
    offset = rs.randn(D) * 0.8
    x_in, g_in = planted(1, 260, D, 20, 6, rot, gains, offset)
    adapt_rows = [i for g in g_in[:160] for i in g]
    return dict(be=be, x_out=x_out, keys=keys, groups=groups, x_in=x_in, adapt=x_in[adapt_rows], eval_groups=g_in[160:230],
                cohort=x_in[[i for g in g_in[230:] for i in g]])


def _eval_trials(w, multi):
    """Enrolment models (multi: averages of up to 3 utterances, else the first utterance), test rows (the last utterance of every speaker with
    >= 2) and every model against every test row."""
    eg = w["eval_groups"]
    e_groups = [g[:max(1, min(3, len(g) - 1))] if multi else g[:1] for g in eg]
    t_spk = [s for s, g in enumerate(eg) if len(g) >= 2]
    t_rows = [eg[s][-1] for s in t_spk]
    ei = np.repeat(np.arange(len(eg)), len(t_spk))
    ti = np.tile(np.arange(len(t_spk)), len(eg))
    targets = ei == np.asarray(t_spk)[ti]
    counts = np.asarray([len(g) for g in e_groups])
    offsets = np.concatenate([[0], np.cumsum(counts)])
    flat = [i for g in e_groups for i in g]
    avg = R.group_means(w["x_in"][flat], D, offsets, np.arange(len(flat))).astype(np.float32)
    return e_groups, t_spk, t_rows, avg, w["x_in"][t_rows], counts, ei, ti, targets


def _model(plda):
    return dict(plda, offset=-(plda["transform"] @ plda["mean"]))


def _llr_bounds(be, eu, te, n_e, tu, tt):
    """For every (model row r, test-role row j): (first-order movement of LLR under the prepared rows' element bounds te / tt, sum of |terms|)."""
    psi = be.plda["psi"][None, None, :]
    n = np.asarray(n_e, dtype=np.float64)[:, None, None]
    a, v = n * psi / (n * psi + 1), 1 + psi / (n * psi + 1)
    diff = tu[None, :, :] - a * eu[:, None, :]
    grad = (np.abs(diff / v) * (tt[None, :, :] + a * te[:, None, :]) + np.abs(tu[None, :, :] / (psi + 1)) * tt[None, :, :]).sum(axis=2)
    terms = (np.abs(0.5 * diff ** 2 / v) + np.abs(0.5 * tu[None, :, :] ** 2 / (psi + 1))).sum(axis=2)
    return grad, terms


def _factored_terms(psi, eu, n_e, cu):
    """[model rows, cohort rows]: the sum of the |terms| of the factored ratio R(e) + C_q(t) + sum_c (iv a e_c) t_c, |k0| included - what the
    bound of the cohort kernel is relative to (csrc/xv_backend_cohort.hip)."""
    counts = sorted(set(int(n) for n in n_e))
    a, iv, g, k0 = R.coefficients(psi, counts)
    q = np.searchsorted(counts, np.asarray(n_e).astype(np.int64))
    return np.abs(iv[q] * a[q] * eu) @ np.abs(cu).T + (0.5 * np.abs(g[None, :] - iv)[q] @ (cu * cu).T) \
        + (0.5 * iv[q] * a[q] ** 2 * eu * eu).sum(axis=1)[:, None] + np.abs(k0)[q][:, None]


def _as_norm_tol(raw, raw_tol, sides, ei, ti):
    """(raw + delta) / sigma + |s - mu| 2 delta / sigma^2 per side, halved and added; sides = ((stats, delta per row), ...) for (enrol, test)."""
    tol = 0.0
    for (st, delta), idx in zip(sides, (ei, ti)):
        mu, sg = st[idx, 0], st[idx, 1]
        tol = tol + 0.5 * ((raw_tol + delta[idx]) / sg + np.abs(raw - mu) * 2 * delta[idx] / sg ** 2)
    return tol


def _kernel_c1(dim):
    return max(2 * ((dim + 3) // 4 * 4) + 2, R.chain(dim) + 3) + 4


def _scoring(be, avg, counts, test, ei, ti, cohort=None, top_k=0, allowance=None):
    """(the restatement's scores through the back end `be`, their bound): raw PLDA, or AS-normed against `cohort`.  allowance None: `be` is
    the model under test bit for bit, the prepared rows' bounds are propagated; a number (MARGIN * Delta_ref): every log-likelihood ratio may
    move by that much and nothing is added for the chain."""
    dim, psi = be.dim, be.plda["psi"]
    eu, tu = A.prepared(be.mean, be.lda, be.plda, avg, counts), A.prepared(be.mean, be.lda, be.plda, test)
    te, tt = _chain_tol(be, avg, counts, True), _chain_tol(be, test, None, True)
    moved = lambda rows_u, rows_t, n_rows, cu, tc: _llr_bounds(be, rows_u, rows_t, n_rows, cu, tc)[0] if allowance is None else allowance
    terms = _llr_bounds(be, eu, te, counts, tu, tt)[1]
    want = R.llr_trials(eu, tu, ei, ti, psi, counts)
    m = moved(eu, te, counts, tu, tt)
    raw_tol = (m[ei, ti] if allowance is None else m) + 2 * (2 * R.chain(dim) + 6) * EPS * terms[ei, ti] + 4 * EPS * np.abs(want)
    if cohort is None:
        return want, raw_tol
    cu, tc = A.prepared(be.mean, be.lda, be.plda, cohort), _chain_tol(be, cohort, None, True)
    normed, raw, e_stats, t_stats = A.as_norm(eu, tu, cu, ei, ti, psi, top_k, counts)
    assert np.abs(raw - want).max() == 0.0
    sides = []
    for rows_u, rows_t, n_rows, st in ((eu, te, counts, e_stats), (tu, tt, np.ones(len(tu), np.int64), t_stats)):
        delta = (moved(rows_u, rows_t, n_rows, cu, tc) + _kernel_c1(dim) * EPS * _factored_terms(psi, rows_u, n_rows, cu)).max(axis=1)
        scores = A.dense_llr(rows_u, cu, psi, n_rows)
        assert np.all(st[:, 1] >= 0.01 * (scores.max(axis=1) - scores.min(axis=1)))      # the deviations are not degenerate (reference alone)
        sides.append((st, delta))
    return normed, _as_norm_tol(raw, raw_tol, sides, ei, ti) + 4 * EPS * np.abs(normed)


def _from_prepared(psi, dim, e, t, c, counts, ei, ti, top_k):
    """AS-normed scores of the rows the GPU prepared (read back, taken in double), and the bound of the kernels alone - no chain in it, so
    a model that met the wrong count, or a test row that met any count but 1, shows.  Trial kernel: its stated bound (csrc/xv_backend.hip);
    cohort kernel: c1 EPS of the factored |terms|; the tables' single roundings (a up to twice in a term, iv, g, k0): 2 EPS of them."""
    e, t, c = (m.cpu().numpy().astype(np.float64)[:, :dim] for m in (e, t, c))
    normed, raw, e_stats, t_stats = A.as_norm(e, t, c, ei, ti, psi, top_k, counts)
    a, v = (lambda n: (n * psi / (n * psi + 1), 1 + psi / (n * psi + 1)))(counts.astype(np.float64)[ei][:, None])
    closed = (np.abs(0.5 * (t[ti] - a * e[ei]) ** 2 / v) + np.abs(0.5 * t[ti] ** 2 / (psi + 1))).sum(axis=1)
    raw_tol = 2 * (2 * R.chain(dim) + 6) * EPS * closed + 2 * EPS * _factored_terms(psi, e, counts, t)[ei, ti] + 2 * EPS * np.abs(raw)
    sides = [(st, ((_kernel_c1(dim) + 2) * EPS * _factored_terms(psi, rows, n, c)).max(axis=1))
             for rows, n, st in ((e, counts, e_stats), (t, np.ones(len(t), np.int64), t_stats))]
    return normed, _as_norm_tol(raw, raw_tol, sides, ei, ti) + 4 * EPS * np.abs(normed)


def _sensitivity(be, adapt, scales, avg, counts, test, ei, ti):
    """(the restatement's adapted back end, Delta_ref): the largest score movement when its scatter statistic moves by the scatter tolerance."""
    from tf_kaldi_speaker_amd.misc import backend as B
    c_blk = _c_blk(len(adapt), DIM)

    def scores(perturb):
        mean_new, plda = A.adapt_backend(be.mean, be.lda, be.plda, adapt, *scales, perturb=perturb)
        ref = B.Backend(mean_new, be.lda, plda)
        eu, tu = A.prepared(ref.mean, ref.lda, ref.plda, avg, counts), A.prepared(ref.mean, ref.lda, ref.plda, test)
        return ref, R.llr_trials(eu, tu, ei, ti, plda["psi"], counts)

    def perturbed(seed):
        rs = np.random.RandomState(seed)

        def perturb(stat, abs_stat):
            sgn = np.triu(rs.choice([-1.0, 1.0], stat.shape))
            return stat + 2 * (c_blk + 2) * EPS * abs_stat * (sgn + np.triu(sgn, 1).T)
        return scores(perturb)[1]

    ref, want = scores(None)
    return ref, want, max(float(np.abs(perturbed(s) - want).max()) for s in (11, 12, 13))


def test_adapt_on_planted_data(world, caplog):
    import logging
    w = world
    be = w["be"]
    scales = (0.75, 0.25, 1.0)
    _, _, _, avg, test, counts, ei, ti, targets = _eval_trials(w, True)
    ref, want, delta_ref = _sensitivity(be, w["adapt"], scales, avg, counts, test, ei, ti)
    s = A.adapt_backend(be.mean, be.lda, be.plda, w["adapt"], *scales)[1]["s"]
    above = int((s > 1.0).sum())
    assert 0 < above < DIM, above                                                 # both branches of the estimator are taken (reference alone)
    with caplog.at_level(logging.INFO, logger="tf_kaldi_speaker_amd"):
        got_be = be.adapt(w["adapt"], device=DEV, within_covar_scale=scales[0], between_covar_scale=scales[1], mean_diff_scale=scales[2])
    assert "PLDA adaptation: N = %d vectors, %d of %d eigenvalues above 1" % (len(w["adapt"]), above, DIM) in caplog.text
    assert np.array_equal(got_be.lda, be.lda) and np.abs(got_be.mean - ref.mean).max() <= 2 * EPS * np.abs(ref.mean).max()
    from tf_kaldi_speaker_amd.misc import backend as B
    sc = B.BackendScorer(got_be, "plda", DEV)
    got = sc.score(sc.prepare(avg, n_utts=counts), sc.prepare(test), ei, ti, enrol_n=counts).astype(np.float64)
    _, tol = _scoring(ref, avg, counts, test, ei, ti, allowance=MARGIN * delta_ref)
    err = np.abs(got - want)
    # the adaptation matters on this data: the unadapted model on the new mean scores differently by far more than the allowance
    base = B.BackendScorer(be.recentred(w["adapt"]), "plda", DEV)
    unadapted = base.score(base.prepare(avg, n_utts=counts), base.prepare(test), ei, ti, enrol_n=counts)
    print("adapt: %d of %d eigenvalues above 1 (s %.3f .. %.3f); Delta_ref %.3e, margin %g, observed max |score difference| %.3e, bound min %.3e; "
          "adapted against unadapted scores differ by up to %.3e; EER reference %.3f%%, GPU %.3f%%, unadapted %.3f%%"
          % (above, DIM, s[0], s[-1], delta_ref, MARGIN, float(err.max()), float(tol.min()), float(np.abs(unadapted - want).max()),
             100 * R.eer(want, targets), 100 * R.eer(got, targets), 100 * R.eer(unadapted, targets)))
    assert np.all(err <= tol), float((err / tol).max())
    assert np.abs(unadapted - want).max() > 10 * tol.max()


def test_backend_scorer_cohort(world):
    """AS-normed PLDA scores, multi-utterance models, a workspace of one 128-row tile as well as the default one."""
    from tf_kaldi_speaker_amd.misc import backend as B
    w = world
    be = w["be"].recentred(w["adapt"])
    _, _, _, avg, test, counts, ei, ti, _ = _eval_trials(w, True)
    avg, counts = np.tile(avg, (3, 1)), np.tile(counts, 3)                       # 210 models: two row tiles under the small workspace
    ei = np.concatenate([ei, ei + 70, ei + 140])
    ti = np.tile(ti, 3)
    want, tol = _scoring(be, avg, counts, test, ei, ti, w["cohort"], 20)
    raw_want, _ = _scoring(be, avg, counts, test, ei, ti)
    n_cohort = len(w["cohort"])
    from tf_kaldi_speaker_amd import ops
    small = ops.backend_plda_cohort_workspace_bytes(128, n_cohort, DIM, len(set(counts) | {1}))
    worst = worst_k = 0.0
    for ws in (B.DEFAULT_WORKSPACE_BYTES, small):
        sc = B.BackendScorer(be, "plda", DEV, workspace_bytes=ws)
        e, t = sc.prepare(avg, n_utts=counts), sc.prepare(test)
        plain = sc.score(e, t, ei, ti, enrol_n=counts)
        sc.cohort(w["cohort"], 20)
        got = sc.score(e, t, ei, ti, enrol_n=counts).astype(np.float64)
        err = np.abs(got - want)
        assert got.shape == want.shape and np.all(err <= tol), float((err / tol).max())
        worst = max(worst, float((err / tol).max()))
        want_k, tol_k = _from_prepared(be.plda["psi"], DIM, e, t, sc.prepare(w["cohort"]), counts, ei, ti, 20)
        assert np.all(np.abs(got - want_k) <= tol_k), float((np.abs(got - want_k) / tol_k).max())
        worst_k = max(worst_k, float((np.abs(got - want_k) / tol_k).max()))
        sc.cohort(None)                                                           # without a cohort nothing changes: the same bits as before it was set
        assert np.array_equal(sc.score(e, t, ei, ti, enrol_n=counts), plain)
    assert np.abs(want - raw_want).max() > 1.0                                    # (the normalisation is not a no-op on this data)
    print("BackendScorer.cohort: %d trials, %d cohort rows, worst error / bound %.5f from raw tables, %.4f from the prepared rows (kernels alone)"
          % (len(ei), n_cohort, worst, worst_k))
    sc = B.BackendScorer(be, "plda", DEV, workspace_bytes=1000)
    sc.cohort(w["cohort"], 20)
    with pytest.raises(ValueError, match="does not hold one 128-row tile"):
        sc.score(sc.prepare(avg, n_utts=counts), sc.prepare(test), ei, ti, enrol_n=counts)
    with pytest.raises(ValueError, match="needs the plda mode"):
        B.BackendScorer(be, "lda_cos", DEV).cohort(w["cohort"], 20)
    with pytest.raises(ValueError, match="top_k must be positive"):
        B.BackendScorer(be, "plda", DEV).cohort(w["cohort"], 0)


# ---- the drivers ------------------------------------------------------------------------------------------------------------------------
def _write_table(path, keys, matrix):
    from tf_kaldi_speaker_amd.dataset import kaldi_io
    with open(path + ".ark", "wb") as f:
        for k, v in zip(keys, matrix):
            kaldi_io.write_vec_flt(f, v, key=k)
    return "ark:%s.ark" % path


def _run(script, args, cwd):
    env = dict(os.environ, TF_KALDI_ROOT=PKG, PYTHONPATH=PKG)
    r = subprocess.run([sys.executable, os.path.join(PKG, "nnet", "lib", script)] + args, env=env, cwd=cwd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (script, r.stderr[-2000:])
    return r


def _read_scores(path, kept):
    lines = open(path).read().splitlines()
    assert [ln.split()[:2] for ln in lines] == [[a, b] for a, b, _ in kept]
    return np.array([float(ln.split()[2]) for ln in lines])


def test_drivers(world, tmp_path):
    """Stage 10 of the SRE recipe through the drivers, each a fresh child process under its own timeout: train_backend.py on the out-of-domain
    table, adapt_backend.py (the recipe's scales) and adapt_backend.py --mean-only true on the in-domain one, then score.py --scoring plda on
    both and --scoring plda_asnorm on the adapted one, with multi-utterance enrolment."""
    from tf_kaldi_speaker_amd.misc import backend as B
    w = world
    tmp = str(tmp_path)
    p = lambda name: os.path.join(tmp, name)
    train_spec = _write_table(p("train"), w["keys"], w["x_out"])
    with open(p("spk2utt"), "w") as f:
        f.write("".join("s%03d %s\n" % (s, " ".join(w["keys"][i] for i in g)) for s, g in enumerate(w["groups"])))
    adapt_spec = _write_table(p("adapt"), ["a%05d" % i for i in range(len(w["adapt"]))], w["adapt"])
    cohort_spec = _write_table(p("cohort"), ["c%04d" % i for i in range(len(w["cohort"]))], w["cohort"])
    _run("train_backend.py", ["--lda-dim", str(DIM), train_spec, p("spk2utt"), p("out_of_domain")], tmp)
    r = _run("adapt_backend.py", ["--within-covar-scale", "0.75", "--between-covar-scale", "0.25", p("out_of_domain"), adapt_spec, p("adapted")], tmp)
    assert re.search(r"PLDA adaptation: N = %d vectors, \d+ of %d eigenvalues above 1 \(largest \S+, smallest \S+\)" % (len(w["adapt"]), DIM), r.stderr)
    _run("adapt_backend.py", ["--mean-only", "true", p("out_of_domain"), adapt_spec, p("recentred")], tmp)
    for name in ("adapted", "recentred"):
        assert sorted(os.listdir(p(name))) == ["mean.vec", "plda", "transform.mat"]
        assert open(os.path.join(p(name), "transform.mat"), "rb").read() == open(os.path.join(p("out_of_domain"), "transform.mat"), "rb").read()
    assert open(os.path.join(p("recentred"), "plda"), "rb").read() == open(os.path.join(p("out_of_domain"), "plda"), "rb").read()
    be = B.Backend.load(p("out_of_domain"))
    # the evaluation: speakers on the enrol side, one listed utterance without a vector, one trial naming a speaker that was not enrolled
    e_groups, t_spk, t_rows, avg, test, counts, ei, ti, targets = _eval_trials(w, True)
    flat = [i for g in e_groups for i in g]
    ukey = lambda i: "e%05d" % i
    e_spec = _write_table(p("enrol"), [ukey(i) for i in flat], w["x_in"][flat])
    t_spec = _write_table(p("test"), ["t%03d" % s for s in t_spk], test)
    with open(p("enrol_spk2utt"), "w") as f:
        f.write("".join("m%03d %s%s\n" % (s, " ".join(ukey(i) for i in g), " e99999" if s == 0 else "") for s, g in enumerate(e_groups)))
    kept = [("m%03d" % a, "t%03d" % t_spk[b], bool(lab)) for a, b, lab in zip(ei, ti, targets)]
    listed = kept[:5] + [("m999", "t%03d" % t_spk[0], False)] + kept[5:]
    with open(p("trials"), "w") as f:
        f.write("".join("%s %s %s\n" % (a, b, "target" if lab else "nontarget") for a, b, lab in listed))
    common = ["--enrol-spk2utt", p("enrol_spk2utt"), p("trials"), e_spec, t_spec, p("scores")]
    ref_adapted, want_adapted, delta_ref = _sensitivity(be, w["adapt"], (0.75, 0.25, 1.0), avg, counts, test, ei, ti)
    eers = {}
    for name, scoring, extra in (("recentred", "plda", []), ("adapted", "plda", []),
                                 ("adapted", "plda_asnorm", ["--cohort", cohort_spec, "--top-k", "20"])):
        r = _run("score.py", ["--backend", p(name), "--scoring", scoring] + extra + common, tmp)
        got = _read_scores(p("scores"), kept)
        assert "Trial m999 t%03d: no vector for a key, skip." % t_spk[0] in r.stderr and "Scored %d trials, skipped 1." % len(kept) in r.stderr
        assert "Utterance e99999 of speaker m000: no vector, skip." in r.stderr
        m = re.search(r"EER ([0-9.]+)%", r.stderr)
        assert m is not None
        eers[(name, scoring)] = float(m.group(1))
        cohort = (w["cohort"], 20) if scoring == "plda_asnorm" else (None, 0)
        if name == "recentred":      # the model is the out-of-domain one bit for bit; only the mean moved
            ref = B.Backend.load(p(name))
            assert np.array_equal(ref.mean, be.recentred(w["adapt"]).mean)
            want, tol = _scoring(ref, avg, counts, test, ei, ti, *cohort)
        else:                        # the adapted model: MARGIN * Delta_ref for every ratio, raw and cohort alike, and no chain term
            want, tol = _scoring(ref_adapted, avg, counts, test, ei, ti, *cohort, allowance=MARGIN * delta_ref)
            if scoring == "plda":
                assert np.abs(want - want_adapted).max() == 0.0
        err = np.abs(got - want)
        assert np.all(err <= tol + 5e-7), (name, scoring, float((err / (tol + 5e-7)).max()))      # (+ the six printed decimals)
        print("drivers %s %s: worst error / bound %.4f (max |error| %.3e, bound min %.3e), EER %.3f%%"
              % (name, scoring, float((err / (tol + 5e-7)).max()), float(err.max()), float(tol.min()), eers[(name, scoring)]))
    # the unchanged command line: --scoring plda on the unadapted directory writes the bytes of BackendScorer without a cohort
    _run("score.py", ["--backend", p("out_of_domain"), "--scoring", "plda"] + common, tmp)
    sc = B.BackendScorer(be, "plda", DEV)
    names, models, n = sc.enrol_average(w["x_in"][flat], [ukey(i) for i in flat], B.read_spk2utt(p("enrol_spk2utt")))
    direct = sc.score(sc.prepare(models, n_utts=n), sc.prepare(test), ei, ti, enrol_n=n)
    assert open(p("scores")).read() == "".join("%s %s %.6f\n" % (a, b, s) for (a, b, _), s in zip(kept, direct))
