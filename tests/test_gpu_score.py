"""The scoring stage on a real MI355X: xv_score_prepare / xv_score_trials / xv_score_cohort_stats through ops.py, CosineScorer and
nnet/lib/score.py against the fp64 restatement (tests/score_ref.py), which reads the same fp32 inputs in double.

Tolerances (EPS = 2^-24, chain(d) = 4 * ceil(d / 256) + 6 as stated in csrc/xv_score.hip):
  trial dot product    2 * (chain(d) + 2) * EPS * sum_c |e_c t_c|, per trial, from the fp64 products
  prepared vectors     2 * (chain(d) + 2) * EPS * sum_c y_c^2 of the reference row (1 for every non-zero row), per element: the relative
                       error of sum v^2 is at most (chain + 3) EPS (every term positive, v itself one rounding off the exact difference of
                       the fp32 inputs), half of which reaches y, plus rsqrt, the subtraction and the product - below 0.5 chain + 6 roundings
  GEMM-backed scores   2e-5 (the project's fp32 GEMM figure for unit-scale outputs); the cohort mean the same: a
                       swap at a near-tie moves the mean by no more than the score error
  cohort deviation     4 * 2e-5 where the reference's deviation is >= 0.01 (asserted on the reference alone for every case with k >= 2 that
                       is not the identical-rows cohort; k = 1 gives the floor 1e-6 on both sides)
  normalised scores    raw tolerance * (1 / sigma_e + 1 / sigma_t) * 2 with the reference's sigma
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import score_ref as R

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
GEMM_TOL = 2e-5
STD_TOL = 4 * GEMM_TOL
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "tf_kaldi_speaker_amd")
DEV = "cuda:0"


def _ops():
    import torch
    from tf_kaldi_speaker_amd import ops
    return torch, ops


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _pitched(torch, a, ld, fill=1e3, offset=0):
    """Device [rows, ld] buffer holding the fp32 matrix a in its leading columns, the padding filled with `fill`; offset: floats the base
    is shifted off the allocation (1: no 16-byte alignment)."""
    rows, d = a.shape
    flat = torch.full((rows * ld + offset,), fill, dtype=torch.float32, device=DEV)
    buf = flat[offset:].view(rows, ld)
    buf[:, :d] = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)
    return buf


def _prepared(torch, a):
    """A prepared-layout device matrix: pitch = d rounded up to 4, zero padding."""
    return _pitched(torch, a, (a.shape[1] + 3) // 4 * 4, fill=0.0)


# ---- prepare ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def prep_data():
    rs = np.random.RandomState(7)
    return (rs.randn(129, 601) * 3 + 0.5).astype(np.float32), rs.randn(601).astype(np.float32)


def _check_prepared(got, x, d, mean, zero_row):
    ref = R.prepare(x, d=d, mean=mean)
    tol = 2 * (R.chain(d) + 2) * EPS * (ref * ref).sum(axis=1, keepdims=True)
    err = np.abs(got[:, :d].astype(np.float64) - ref)
    assert np.all(err <= tol), (d, float((err / np.maximum(tol, 1e-300)).max()))
    assert np.all(got[:, d:] == 0.0)                        # the padding comes back zero (it went in as 1e3)
    if zero_row is not None:
        assert np.all(got[zero_row] == 0.0) and np.all(ref[zero_row] == 0.0)
    return float((err / np.maximum(tol, 1e-300)).max())


@pytest.mark.parametrize("with_mean", [False, True])
@pytest.mark.parametrize("rows", [1, 3, 129])
@pytest.mark.parametrize("d", [1, 30, 512, 601])
def test_prepare(prep_data, d, rows, with_mean):
    torch, ops = _ops()
    xs, means = prep_data
    x = xs[:rows, :d].copy()
    mean = means[:d].copy() if with_mean else None
    zero_row = rows // 2 if rows >= 3 else None
    if zero_row is not None:
        x[zero_row] = mean if with_mean else 0.0
    mean_d = torch.from_numpy(mean).to(DEV) if with_mean else None
    d4 = (d + 3) // 4 * 4
    worst = 0.0
    # pitches on the 16-byte grid (vector loads when d is a multiple of 4), then a base and pitches off it (the scalar path)
    for ldx, ldy, off in ((d4 + 4, d4 + 8, 0), (d + 1, d + 3, 1)):
        xb = _pitched(torch, x, ldx, offset=off)
        out = _pitched(torch, np.zeros((rows, 0), np.float32), ldy, offset=off)
        got = ops.score_prepare(xb, d=d, mean=mean_d, out=out)
        assert got.data_ptr() == out.data_ptr()
        worst = max(worst, _check_prepared(got.cpu().numpy(), x, d, mean, zero_row))
        assert np.all(xb.cpu().numpy()[:, d:] == 1e3)      # the input's padding is neither read into a norm nor written
    print("prepare d=%d rows=%d mean=%s: worst error / bound %.3f" % (d, rows, with_mean, worst))


@pytest.mark.parametrize("d,ld", [(512, 520), (30, 33)])
def test_prepare_in_place_and_default_output(prep_data, d, ld):
    torch, ops = _ops()
    xs, means = prep_data
    x = xs[:129, :d].copy()
    mean_d = torch.from_numpy(means[:d].copy()).to(DEV)
    buf = _pitched(torch, x, ld)
    got = ops.score_prepare(buf, d=d, mean=mean_d, out=buf)
    assert got.data_ptr() == buf.data_ptr()
    _check_prepared(buf.cpu().numpy(), x, d, means[:d], None)
    fresh = ops.score_prepare(torch.from_numpy(x).to(DEV), mean=mean_d)          # default: a new matrix on the pitch d rounded up to 4
    assert tuple(fresh.shape) == (129, (d + 3) // 4 * 4)
    _check_prepared(fresh.cpu().numpy(), x, d, means[:d], None)
    from tf_kaldi_speaker_amd._lib import XvError
    with pytest.raises(XvError, match="x and y overlap"):
        ops.score_prepare(buf[:128], d=d, out=buf[1:])      # y one row into x: not in place


# ---- trials ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trial_data():
    rs = np.random.RandomState(11)
    e = _unit(rs.randn(7, 512)).astype(np.float32)
    t = _unit(rs.randn(5, 512)).astype(np.float32)
    e_stats = np.stack([rs.uniform(-0.1, 0.2, 7), rs.uniform(0.05, 0.2, 7)], axis=1).astype(np.float32)
    t_stats = np.stack([rs.uniform(-0.1, 0.2, 5), rs.uniform(0.05, 0.2, 5)], axis=1).astype(np.float32)
    return e, t, e_stats, t_stats


def _trial_indices(m, ne, nt):
    rs = np.random.RandomState(m)
    ei = (np.arange(m)[::-1] % ne).astype(np.int64)         # reversed and, beyond ne trials, repeated
    ti = rs.randint(0, nt, m)
    if m >= 3:
        ei[1], ti[1] = ei[0], ti[0]                         # one trial twice in a row
    return ei, ti


def _raw_tol(e, t, ei, ti, d):
    return 2 * (R.chain(d) + 2) * EPS * np.abs(e[ei].astype(np.float64)[:, :d] * t[ti].astype(np.float64)[:, :d]).sum(axis=1)


@pytest.mark.parametrize("d", [512, 30])
@pytest.mark.parametrize("m", [1, 63, 64, 65, 1000])
def test_trials(trial_data, m, d):
    torch, ops = _ops()
    e, t, e_stats, t_stats = trial_data
    e, t = e[:, :d], t[:, :d]
    ei, ti = _trial_indices(m, 7, 5)
    # d = 512: 16-byte grid (vector loads); d = 30: the scalar path, the padding (1e3) must not enter a sum on either
    eb, tb = _pitched(torch, e, d + (4 if d % 4 == 0 else 3)), _pitched(torch, t, d + (8 if d % 4 == 0 else 1))
    tol = _raw_tol(e, t, ei, ti, d)
    got = ops.score_trials(eb, tb, d, ei, ti).cpu().numpy().astype(np.float64)
    err = np.abs(got - R.trials(e, t, ei, ti))
    assert got.shape == (m,) and np.all(err <= tol), float((err / tol).max())
    es, ts = torch.from_numpy(e_stats).to(DEV), torch.from_numpy(t_stats).to(DEV)
    got_n = ops.score_trials(eb, tb, d, ei, ti, es, ts).cpu().numpy().astype(np.float64)
    tol_n = tol * (1.0 / e_stats[ei, 1].astype(np.float64) + 1.0 / t_stats[ti, 1].astype(np.float64)) * 2
    err_n = np.abs(got_n - R.trials(e, t, ei, ti, e_stats, t_stats))
    assert np.all(err_n <= tol_n), float((err_n / tol_n).max())
    print("trials m=%d d=%d: worst error / bound raw %.3f normalised %.3f" % (m, d, (err / tol).max(), (err_n / tol_n).max()))


def test_trials_refusals(trial_data):
    torch, ops = _ops()
    from tf_kaldi_speaker_amd._lib import XvError
    e, t, e_stats, _ = trial_data
    eb, tb = _prepared(torch, e), _prepared(torch, t)
    with pytest.raises(IndexError, match="ei holds an index outside 0 .. 6"):
        ops.score_trials(eb, tb, 512, [0, 7], [0, 0])
    with pytest.raises(IndexError, match="ti holds an index outside 0 .. 4"):
        ops.score_trials(eb, tb, 512, [0, 1], [0, -1])
    with pytest.raises(IndexError, match="ti holds an index outside"):
        ops.score_trials(eb, tb, 512, [6], [5])                                     # ne != nt: an enrol index is not a test index
    with pytest.raises(XvError, match="both be given or both be NULL"):
        ops.score_trials(eb, tb, 512, [0], [0], e_stats=torch.from_numpy(e_stats).to(DEV))


# ---- cohort statistics -----------------------------------------------------------------------------------------------------------------
COHORT_SIZES = [1, 5, 255, 256, 257, 4097]


def _designed(rs, rows, n, d):
    """Prepared rows x near one direction u and a cohort whose first eight rows meet u at cosines 1, 0.88, 0.76, ... (the rest are random
    unit vectors, cosine ~ N(0, 1/d) with x): the top scores of every row are 0.1 apart, so the deviation of any top-k >= 2 is far above
    the 0.01 the tolerance needs."""
    u = _unit(rs.randn(d))
    x = _unit(u + 0.1 * rs.randn(rows, d) / np.sqrt(d))
    c = _unit(rs.randn(n, d))
    for j in range(min(n, 8)):
        w = rs.randn(d)
        w = _unit(w - (w @ u) * u)
        a = 1.0 - 0.12 * j
        c[j] = a * u + np.sqrt(1.0 - a * a) * w
    return x.astype(np.float32), c.astype(np.float32)


@pytest.fixture(scope="module")
def cohort_data():
    """x [130, 64], the cohort [4097, 64] (smaller cohorts take its leading rows) and the fp64 scores; computed once, read only."""
    x, c = _designed(np.random.RandomState(5), 130, 4097, 64)
    scores = R.cohort_scores(x, c)
    scores.setflags(write=False)
    return x, c, scores


def _check_stats(got, ref, degenerate=False):
    got = got.astype(np.float64)
    assert np.all(np.isfinite(got))
    if not degenerate:
        assert ref[:, 1].min() >= 0.01, ref[:, 1].min()
    e_mean, e_std = np.abs(got[:, 0] - ref[:, 0]).max(), np.abs(got[:, 1] - ref[:, 1]).max()
    print("cohort statistics: worst |mean error| %.2e |deviation error| %.2e" % (e_mean, e_std))
    assert e_mean <= GEMM_TOL and e_std <= STD_TOL, (e_mean, e_std)
    return e_mean, e_std


@pytest.mark.parametrize("rows", [1, 130])
@pytest.mark.parametrize("n_cohort", COHORT_SIZES)
def test_cohort_stats(cohort_data, n_cohort, rows):
    torch, ops = _ops()
    x, c, scores = cohort_data
    xb, cb = _prepared(torch, x[:rows]), _prepared(torch, c[:n_cohort])
    worst = (0.0, 0.0)
    for top_k in sorted({1, 2, n_cohort - 1, n_cohort, n_cohort + 7}):
        if top_k <= 0:
            continue                                        # (n_cohort = 1: top_k = 0 is a refusal, test_cohort_refusals)
        got = ops.score_cohort_stats(xb, cb, 64, top_k).cpu().numpy()
        ref = R.top_k_stats(scores[:rows, :n_cohort], top_k)
        k = min(top_k, n_cohort)
        if k == 1:
            assert np.all(ref[:, 1] == 1e-6)
        worst = tuple(np.maximum(worst, _check_stats(got, ref, degenerate=k == 1)))
    print("cohort n=%d rows=%d: worst |mean error| %.2e |deviation error| %.2e" % ((n_cohort, rows) + worst))


def test_cohort_two_row_tiles_from_a_one_tile_workspace(cohort_data):
    """130 rows through a workspace of exactly one 128-row tile: two GEMM + select rounds."""
    torch, ops = _ops()
    x, c, scores = cohort_data
    xb, cb = _prepared(torch, x), _prepared(torch, c[:257])
    one_tile = ops.score_cohort_workspace_bytes(128, 257, 64)
    assert one_tile == 128 * 260 * 4 and ops.score_cohort_workspace_bytes(130, 257, 64) == 2 * one_tile
    got = ops.score_cohort_stats(xb, cb, 64, 20, ws_bytes=one_tile)
    _check_stats(got.cpu().numpy(), R.top_k_stats(scores[:, :257], 20))


def test_cohort_odd_dimension_and_long_rows():
    """d = 30 (the GEMM reads the two zero columns up to 32) and d = 512 (the evaluation size: 32 K-steps)."""
    torch, ops = _ops()
    for d, seed in ((30, 1), (512, 2)):
        x, c = _designed(np.random.RandomState(seed), 130, 257, d)
        got = ops.score_cohort_stats(_prepared(torch, x), _prepared(torch, c), d, 20).cpu().numpy()
        _check_stats(got, R.cohort_stats(x, c, 20))


def test_cohort_ties_negative_scores_and_identical_rows():
    torch, ops = _ops()
    rs = np.random.RandomState(9)
    # every cohort row four times: top_k = 6 takes the best run whole and cuts the second one in half
    x, base = _designed(rs, 130, 10, 64)
    c = np.repeat(base, 4, axis=0)
    ref = R.cohort_stats(x, c, 6)
    s = R.cohort_scores(x, c)
    top = -np.sort(-s, axis=1)
    assert np.all(top[:, 3] > top[:, 4] + 0.01) and np.all(top[:, 4] - top[:, 7] <= 1e-14)      # the cut (after 6) falls inside a run of equal scores
    _check_stats(ops.score_cohort_stats(_prepared(torch, x), _prepared(torch, c), 64, 6).cpu().numpy(), ref)
    # every score negative: the cohort on the far side of u, cosines -1 ... -0.3
    u = _unit(rs.randn(64))
    xn = _unit(u + 0.1 * rs.randn(3, 64) / 8.0).astype(np.float32)
    a = np.linspace(0.3, 1.0, 100)[:, None]
    w = rs.randn(100, 64)
    w = _unit(w - (w @ u)[:, None] * u)
    cn = (-(a * u + np.sqrt(1.0 - a * a) * w)).astype(np.float32)
    assert R.cohort_scores(xn, cn).max() < -0.2
    _check_stats(ops.score_cohort_stats(_prepared(torch, xn), _prepared(torch, cn), 64, 10).cpu().numpy(), R.cohort_stats(xn, cn, 10))
    # a cohort of identical rows: the deviation is the floor (or rounding noise), never NaN
    ci = np.repeat(base[1:2], 37, axis=0)
    got = ops.score_cohort_stats(_prepared(torch, x), _prepared(torch, ci), 64, 5).cpu().numpy().astype(np.float64)
    ref = R.cohort_stats(x, ci, 5)
    assert np.all(np.isfinite(got)) and np.abs(got[:, 0] - ref[:, 0]).max() <= GEMM_TOL and np.all(got[:, 1] <= GEMM_TOL)


def test_cohort_refusals(cohort_data):
    torch, ops = _ops()
    from tf_kaldi_speaker_amd._lib import XvError
    x, c, _ = cohort_data
    xb, cb = _prepared(torch, x[:4]), _prepared(torch, c[:5])
    with pytest.raises(XvError, match="top_k must be positive"):
        ops.score_cohort_stats(xb, cb, 64, 0)
    with pytest.raises(XvError, match="n_cohort must be positive"):
        ops.score_cohort_stats(xb, cb[:0], 64, 2)
    with pytest.raises(XvError, match="at least one 128-row tile"):
        ops.score_cohort_stats(xb, cb, 64, 2, ws_bytes=128 * 8 * 4 - 4)
    with pytest.raises(XvError, match="both pitches must reach d rounded up to 4"):
        ops.score_cohort_stats(_pitched(torch, x[:4, :30], 30), cb, 30, 2)
    with pytest.raises(XvError, match="gemm_nt: K/lda/ldb must be multiples of 4"):      # what the GEMM refuses, in its words
        ops.score_cohort_stats(_pitched(torch, x[:4], 66, fill=0.0), cb, 64, 2)
    with pytest.raises(XvError, match="gemm_nt: operands must be 16-byte aligned"):
        ops.score_cohort_stats(_pitched(torch, x[:4], 64, offset=1), cb, 64, 2)


# ---- determinism -----------------------------------------------------------------------------------------------------------------------
def test_two_calls_are_bit_identical(cohort_data, trial_data, prep_data):
    torch, ops = _ops()
    x, c, _ = cohort_data
    xb, cb = _prepared(torch, x), _prepared(torch, c)
    assert torch.equal(ops.score_cohort_stats(xb, cb, 64, 300), ops.score_cohort_stats(xb, cb, 64, 300))
    e, t, e_stats, t_stats = trial_data
    eb, tb = _prepared(torch, e), _prepared(torch, t)
    es, ts = torch.from_numpy(e_stats).to(DEV), torch.from_numpy(t_stats).to(DEV)
    ei, ti = _trial_indices(1000, 7, 5)
    assert torch.equal(ops.score_trials(eb, tb, 512, ei, ti, es, ts), ops.score_trials(eb, tb, 512, ei, ti, es, ts))
    xs, means = prep_data
    for d in (512, 601):
        xd, md = torch.from_numpy(xs[:, :d].copy()).to(DEV), torch.from_numpy(means[:d].copy()).to(DEV)
        assert torch.equal(ops.score_prepare(xd, mean=md), ops.score_prepare(xd, mean=md))


# ---- CosineScorer and the driver -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tables():
    """Small raw embedding tables (d = 24, nothing centred or normalised yet) with a speaker structure, a cohort and a trial list."""
    rs = np.random.RandomState(17)
    spk = rs.randn(6, 24) * 2.0
    offset = rs.randn(24) * 1.5                             # a common offset: what --center-on removes
    enrol = (spk[np.arange(18) % 6] + rs.randn(18, 24) + offset).astype(np.float32)
    test = (spk[np.arange(15) % 6] + rs.randn(15, 24) + offset).astype(np.float32)
    cohort = (rs.randn(12, 24) * 2.0 + rs.randn(12, 24) + offset).astype(np.float32)
    ekeys, tkeys = ["e%02d" % i for i in range(18)], ["t%02d" % i for i in range(15)]
    pairs = [(int(a), int(b)) for a, b in zip(rs.randint(0, 18, 60), rs.randint(0, 15, 60))]
    return dict(enrol=enrol, test=test, cohort=cohort, ekeys=ekeys, tkeys=tkeys, pairs=pairs)


def _pipeline_tol(enrol, test, ei, ti, center, cohort, top_k):
    """Bound on |score - reference| for the whole pipeline from raw tables, from the op-level figures.  A prepared row is off by at most
    p = 2 (chain(d) + 2) EPS per element, so any dot product with a unit vector by at most sqrt(d) p per prepared operand: in = 2 sqrt(d) p.
    Raw score: in + the trial sum's own bound (at most p: sum |e_c t_c| <= 1).  Cohort score and mean: in + 2e-5; deviation: 4 times that.
    Normalised: each half (s - mu) / sigma moves by (d s + d mu) / sigma + |s - mu| d sigma / sigma^2."""
    d = enrol.shape[1]
    p = 2 * (R.chain(d) + 2) * EPS
    t_in = 2 * np.sqrt(d) * p
    raw = t_in + p
    if cohort is None:
        return np.full(len(ei), raw)
    e, t, c = R.prepare(enrol, mean=center), R.prepare(test, mean=center), R.prepare(cohort, mean=center)
    s = R.trials(e, t, ei, ti)
    tol = 0.0
    for st, idx in ((R.cohort_stats(e, c, top_k), ei), (R.cohort_stats(t, c, top_k), ti)):
        assert st[:, 1].min() >= 0.01
        mu, sg = st[idx, 0], st[idx, 1]
        tol = tol + 0.5 * ((raw + t_in + GEMM_TOL) / sg + np.abs(s - mu) * 4 * (t_in + GEMM_TOL) / sg ** 2)
    return tol


def test_cosine_scorer_batches_inside_its_workspace(tables):
    """CosineScorer with the default workspace and with one that holds a single 128-row cohort tile and 512 trials a call (144 enrolment
    rows: two row batches; 600 trials: two trial batches): both within the bound."""
    from tf_kaldi_speaker_amd.misc import scoring
    T = tables
    enrol = np.tile(T["enrol"], (8, 1))
    ei = np.tile([p[0] for p in T["pairs"]], 10) + 18 * (np.arange(600) % 8)
    ti = np.tile([p[1] for p in T["pairs"]], 10)
    center = scoring.center_mean(T["cohort"])
    want = R.score_pipeline(enrol, T["test"], ei, ti, center=center.astype(np.float32), cohort=T["cohort"], top_k=5)
    tol = _pipeline_tol(enrol, T["test"], ei, ti, center.astype(np.float32), T["cohort"], 5)
    for ws in (scoring.DEFAULT_WORKSPACE_BYTES, 128 * 12 * 4):
        sc = scoring.CosineScorer(DEV, center=center, workspace_bytes=ws)
        e, t = sc.prepare(enrol), sc.prepare(T["test"])
        sc.cohort(T["cohort"], 5)
        got = sc.score(e, t, ei, ti)
        assert got.shape == (600,) and np.all(np.abs(got - want) <= tol), float((np.abs(got - want) / tol).max())
    sc = scoring.CosineScorer(DEV, workspace_bytes=100)
    sc.cohort(T["cohort"], 5)
    with pytest.raises(ValueError, match="does not hold one 128-row tile"):
        sc.score(sc.prepare(T["enrol"]), sc.prepare(T["test"]), ei % 18, ti)
    with pytest.raises(ValueError, match="dimension mismatch"):
        sc.prepare(T["enrol"][:, :20])


def _write_table(path, keys, matrix, scp=False):
    from tf_kaldi_speaker_amd.dataset import kaldi_io
    with open(path + ".ark", "wb") as f, open(path + ".scp", "w") as s:
        for k, v in zip(keys, matrix):
            s.write("%s %s.ark:%d\n" % (k, path, f.tell() + len(k) + 1))
            kaldi_io.write_vec_flt(f, v, key=k)
    return ("scp:%s.scp" if scp else "ark:%s.ark") % path


def _run_driver(args, cwd):
    env = dict(os.environ, TF_KALDI_ROOT=PKG, PYTHONPATH=PKG)
    r = subprocess.run([sys.executable, os.path.join(PKG, "nnet", "lib", "score.py")] + args, env=env, cwd=cwd, capture_output=True, text=True,
                       timeout=300)
    return r


def _check_driver_output(r, out_path, kept, want, tol, skipped, labelled):
    from tf_kaldi_speaker_amd.misc import scoring
    assert r.returncode == 0, r.stderr[-2000:]
    lines = open(out_path).read().splitlines()
    assert [ln.split()[:2] for ln in lines] == [[a, b] for a, b, _ in kept]               # every kept trial, in trial order
    got = np.array([float(ln.split()[2]) for ln in lines])
    assert np.all(np.abs(got - want) <= tol + 5e-7), float(np.abs(got - want).max())      # (+ the six printed decimals)
    assert "Scored %d trials, skipped %d." % (len(kept), skipped) in r.stderr
    m = re.search(r"EER ([0-9.]+)%  minDCF08 ([0-9.]+)  minDCF10 ([0-9.]+)", r.stderr)
    assert (m is not None) == labelled
    if labelled:
        targets = np.array([lab for _, _, lab in kept])
        # the EER depends on the order of the scores alone: the reference's scores are further apart than twice the bound wherever a
        # target meets a nontarget, so both sides sort alike and the printed figure is the reference's to its four decimals
        order = np.argsort(want)
        mixed = targets[order][1:] != targets[order][:-1]
        assert np.all((np.diff(want[order]) > 2 * np.maximum(tol[order][1:], tol[order][:-1]) + 1e-6)[mixed])
        assert abs(float(m.group(1)) - 100.0 * scoring.compute_eer(want, targets.astype(np.float64))) <= 1e-4
        for g, name in ((2, "minDCF08"), (3, "minDCF10")):
            assert abs(float(m.group(g)) - scoring.compute_min_dcf(want, targets, *scoring.MIN_DCF_PRESETS[name])) <= 1e-4


def test_driver_same_archive_raw_cosine(tables, tmp_path):
    """score.py trials ark:x ark:x out - one table on both sides, no centring, no cohort, labelled trials -> scores, order and EER."""
    T = tables
    spec = _write_table(str(tmp_path / "emb"), T["ekeys"], T["enrol"])
    pairs = [(a, b % 18) for a, b in T["pairs"] if a != b % 18]
    kept = [(T["ekeys"][a], T["ekeys"][b], a % 6 == b % 6) for a, b in pairs]
    with open(tmp_path / "trials", "w") as f:
        f.write("".join("%s %s %s\n" % (a, b, "target" if lab else "nontarget") for a, b, lab in kept))
    out = str(tmp_path / "scores")
    r = _run_driver([str(tmp_path / "trials"), spec, spec, out], str(tmp_path))
    ei, ti = np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs])
    want = R.score_pipeline(T["enrol"], T["enrol"], ei, ti)
    _check_driver_output(r, out, kept, want, _pipeline_tol(T["enrol"], T["enrol"], ei, ti, None, None, 0), 0, True)


def test_driver_two_archives_centred_as_norm_and_a_missing_key(tables, tmp_path):
    """score.py --center-on scp:cohort --cohort scp:cohort --top-k 5 trials scp:enrol ark:test out, one trial naming a key that is not
    there: logged, skipped, counted; everything else in order.  Then a test table of another dimension: refused by name."""
    from tf_kaldi_speaker_amd.misc import scoring
    T = tables
    e_spec = _write_table(str(tmp_path / "enrol"), T["ekeys"], T["enrol"], scp=True)
    t_spec = _write_table(str(tmp_path / "test"), T["tkeys"], T["test"])
    c_spec = _write_table(str(tmp_path / "cohort"), ["c%d" % i for i in range(12)], T["cohort"], scp=True)
    kept = [(T["ekeys"][a], T["tkeys"][b], a % 6 == b % 6) for a, b in T["pairs"]]
    listed = kept[:7] + [("e03", "t99", False)] + kept[7:]
    with open(tmp_path / "trials", "w") as f:
        f.write("".join("%s %s %s\n" % (a, b, "target" if lab else "nontarget") for a, b, lab in listed))
    out = str(tmp_path / "scores")
    r = _run_driver(["--center-on", c_spec, "--cohort", c_spec, "--top-k", "5", str(tmp_path / "trials"), e_spec, t_spec, out], str(tmp_path))
    ei, ti = np.array([p[0] for p in T["pairs"]]), np.array([p[1] for p in T["pairs"]])
    center = scoring.center_mean(T["cohort"]).astype(np.float32)
    want = R.score_pipeline(T["enrol"], T["test"], ei, ti, center=center, cohort=T["cohort"], top_k=5)
    tol = _pipeline_tol(T["enrol"], T["test"], ei, ti, center, T["cohort"], 5)
    _check_driver_output(r, out, kept, want, tol, 1, True)
    assert "Trial e03 t99: no vector for a key, skip." in r.stderr
    with open(tmp_path / "trials2", "w") as f:
        f.write("".join("%s %s\n" % (a, b) for a, b, _ in listed))
    t5 = _write_table(str(tmp_path / "test5"), T["tkeys"], T["test"][:, :5])
    r = _run_driver([str(tmp_path / "trials2"), e_spec, t5, out], str(tmp_path))
    assert r.returncode != 0 and "dimension mismatch: enrol_rspecifier holds vectors of 24 dimensions, test_rspecifier of 5" in r.stderr
