"""The dense score matrices of one recording on a real MI355X: xv_score_dense and xv_backend_plda_dense through ops.py, written into views
of a packed buffer, against fp64 arithmetic on the same fp32 inputs.

Tolerances (EPS = 2^-24, kd = d rounded up to 4).  score_dense is one GEMM sum: each of its kd steps, in whatever order the GEMM takes its
K, rounds at most twice and every partial sum is bounded by sum_c |x_c y_c| - (2 kd + 2) EPS sum_c |x_c y_c|, the GEMM line of the budget
in csrc/xv_backend_cohort.hip.  backend_plda_dense is that unit's element v(r, j) = (slab + C[j]) + R[r] with one table entry: its c1 budget,
as tests/test_gpu_plda_cohort.py asserts it; against ops.backend_plda_trials on all pairs the two budgets add (tests/test_gpu_backend.py
states the trial kernel's)."""
import numpy as np
import pytest

from tests import backend_ref as R

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
DEV = "cuda:0"
SIZES = (1, 5, 129, 300)
DIMS = (6, 200)


def _ops():
    import torch
    from tf_kaldi_speaker_amd import ops
    return torch, ops


def _prepared(torch, a):
    rows, d = a.shape
    buf = torch.zeros((rows, (d + 3) // 4 * 4), dtype=torch.float32, device=DEV)
    buf[:, :d] = torch.from_numpy(np.array(a, dtype=np.float32)).to(DEV)      # (a copy: the cases are read-only)
    return buf


def _view(torch, n, lead, ld):
    """A [n, n] view of pitch ld, `lead` floats into a NaN-filled buffer: (buffer, view)."""
    buf = torch.full((lead + n * ld + 7,), float("nan"), dtype=torch.float32, device=DEV)
    return buf, buf[lead:lead + n * ld].view(n, ld)[:, :n]


def _untouched(buf, n, lead, ld):
    """Everything of the buffer outside the view's n columns is still NaN."""
    host = buf.cpu().numpy()
    mask = np.ones(host.shape, bool)
    body = mask[lead:lead + n * ld].reshape(n, ld)
    body[:, :n] = False
    return bool(np.isnan(host[mask]).all()) and not bool(np.isnan(host[~mask]).any())


_CASES = {}


def _case(d):
    """Rows of 300 'recording windows' at dimension d, cosine and PLDA flavour, with their fp64 references; built once, read only."""
    if d not in _CASES:
        from tf_kaldi_speaker_amd.misc import backend as B
        rs = np.random.RandomState(7 + d)
        n = max(SIZES)
        spk = rs.randn(4, d)
        unit = spk[rs.randint(0, 4, n)] + 0.5 * rs.randn(n, d)
        unit = (unit / np.linalg.norm(unit, axis=1, keepdims=True)).astype(np.float32)
        psi = np.sort(rs.uniform(0.05, 5.0, d))[::-1].copy()
        y = ((spk * np.sqrt(psi))[rs.randint(0, 4, n)] + rs.randn(n, d)).astype(np.float32)
        y = R.plda_normalize(y.astype(np.float64), psi).astype(np.float32)      # one utterance per row
        coef, g, k0 = B.plda_coefficients(psi, [1])
        u64 = unit.astype(np.float64)
        c = dict(d=d, kd=(d + 3) // 4 * 4, unit=unit, cos=u64 @ u64.T, cos_abs=np.abs(u64) @ np.abs(u64).T, y=y, coef=coef, g=g, k0=k0)
        # every pair as a trial (e = row r in the model role, t = row j), fp64 on the fp32 tables, and the |terms| of the factored form
        tj = np.arange(n)
        rows = [R.trials_from_tables(y, y, np.full(n, r), tj, np.zeros(n, np.int64), coef, g, k0, d) for r in range(n)]
        c["llr"] = np.stack([w for w, _, _ in rows])
        c["trial_tol"] = np.stack([2 * (2 * R.chain(d) + 6) * EPS * terms + EPS * np.abs(k0q) for _, terms, k0q in rows])
        a, iv, gg = (t.astype(np.float64)[..., :d] for t in (coef[0, 0], coef[0, 1], g))
        y64 = y.astype(np.float64)
        gemm = np.abs(iv * a * y64) @ np.abs(y64).T
        cterm = (0.5 * np.abs(gg - iv) * (y64 * y64)).sum(axis=1)
        rterm = (0.5 * iv * a ** 2 * y64 * y64).sum(axis=1)
        c1 = max(2 * c["kd"] + 2, R.chain(d) + 3) + 4
        c["dense_tol"] = c1 * EPS * (gemm + cterm[None, :] + rterm[:, None] + abs(float(k0[0])))
        for v in c.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _CASES[d] = c
    return _CASES[d]


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("n", SIZES)
def test_score_dense(n, d):
    torch, ops = _ops()
    c = _case(d)
    x = _prepared(torch, c["unit"][:n])
    tol = (2 * c["kd"] + 2) * EPS * c["cos_abs"][:n, :n]
    worst = 0.0
    for lead, ld in ((0, (n + 3) // 4 * 4), (3, n + 1), (8, n)):      # on the 16-byte grid, off it, and a pitch of exactly n
        buf, view = _view(torch, n, lead, ld)
        got = ops.score_dense(x, d, out=view)
        assert got.data_ptr() == view.data_ptr() and _untouched(buf, n, lead, ld)
        err = np.abs(got.cpu().numpy().astype(np.float64) - c["cos"][:n, :n])
        worst = max(worst, float((err / tol).max()))
        print("score_dense n=%d d=%d lead=%d ld=%d: worst error / bound %.4f" % (n, d, lead, ld, float((err / tol).max())))
        assert np.all(err <= tol), worst
    new = ops.score_dense(x, d)
    assert tuple(new.shape) == (n, n) and np.all(np.abs(new.cpu().numpy().astype(np.float64) - c["cos"][:n, :n]) <= tol)


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("n", SIZES)
def test_backend_plda_dense(n, d):
    torch, ops = _ops()
    c = _case(d)
    x = _prepared(torch, c["y"][:n])
    tabs = tuple(torch.from_numpy(np.array(t)).to(DEV) for t in (c["coef"], c["g"], c["k0"]))
    tol = c["dense_tol"][:n, :n]
    ei, ti = (a.reshape(-1) for a in np.meshgrid(np.arange(n), np.arange(n), indexing="ij"))
    trials = ops.backend_plda_trials(x, x, d, ei, ti, np.zeros(n, np.int64), *tabs).cpu().numpy().astype(np.float64).reshape(n, n)
    for lead, ld in ((0, (n + 3) // 4 * 4), (3, n + 1)):
        buf, view = _view(torch, n, lead, ld)
        got = ops.backend_plda_dense(x, d, *tabs, out=view)
        assert got.data_ptr() == view.data_ptr() and _untouched(buf, n, lead, ld)
        got = got.cpu().numpy().astype(np.float64)
        err = np.abs(got - c["llr"][:n, :n])
        print("backend_plda_dense n=%d d=%d lead=%d ld=%d: worst error / c1 budget %.4f; against plda_trials / both budgets %.4f"
              % (n, d, lead, ld, float((err / tol).max()), float((np.abs(got - trials) / (tol + c["trial_tol"][:n, :n])).max())))
        assert np.all(err <= tol)
        assert np.all(np.abs(got - trials) <= tol + c["trial_tol"][:n, :n])
    again = ops.backend_plda_dense(x, d, *tabs)
    assert np.array_equal(again.cpu().numpy().view(np.int32), view.cpu().numpy().view(np.int32))      # the same bits whatever the pitch of out


def test_scorers_dense_in_every_mode():
    """CosineScorer.dense and BackendScorer.dense (lda_cos: the cosine behind the LDA, plda: the ratio) are the ops on the scorers' prepared rows."""
    torch, ops = _ops()
    from tf_kaldi_speaker_amd.misc import backend as B
    from tf_kaldi_speaker_amd.misc import scoring as S
    rs = np.random.RandomState(3)
    d, dim, n = 24, 10, 37
    x = rs.randn(n, d).astype(np.float32)
    plda = dict(mean=0.1 * rs.randn(dim), transform=np.linalg.qr(rs.randn(dim, dim))[0], psi=np.sort(rs.uniform(0.1, 4.0, dim))[::-1].copy())
    backend = B.Backend(x.mean(axis=0), np.concatenate([rs.randn(dim, d) * 0.3, rs.randn(dim, 1) * 0.1], axis=1).astype(np.float32), plda)
    cos = S.CosineScorer(DEV, center=x.mean(axis=0))
    p = cos.prepare(x)
    assert torch.equal(cos.dense(p), ops.score_dense(p, d))
    lda = B.BackendScorer(backend, "lda_cos", DEV)
    p = lda.prepare(x)
    got = lda.dense(p).cpu().numpy()
    assert np.allclose(np.diag(got), 1.0, atol=1e-5) and np.abs(got).max() <= 1.0 + 1e-5
    full = B.BackendScorer(backend, "plda", DEV)
    p = full.prepare(x)
    ei, ti = (a.reshape(-1) for a in np.meshgrid(np.arange(n), np.arange(n), indexing="ij"))
    want = full.score(p, p, ei, ti).reshape(n, n)
    got = full.dense(p).cpu().numpy()
    assert np.all(np.abs(got - want) <= 1e-4 * (1.0 + np.abs(want)))      # (the budgets proper: test_backend_plda_dense)
    buf, view = _view(torch, n, 5, n + 2)
    assert full.dense(p, out=view).data_ptr() == view.data_ptr() and np.array_equal(view.cpu().numpy().view(np.int32), got.view(np.int32))


def test_refusals():
    torch, ops = _ops()
    from tf_kaldi_speaker_amd._lib import XvError
    c = _case(6)
    x = _prepared(torch, c["unit"][:5])
    tabs = tuple(torch.from_numpy(np.array(t)).to(DEV) for t in (c["coef"], c["g"], c["k0"]))
    with pytest.raises(ValueError, match=r"out must be a float32 \[5, 5\] view"):
        ops.score_dense(x, 6, out=torch.zeros((5, 4), dtype=torch.float32, device=DEV))
    with pytest.raises(ValueError, match=r"out must be a float32 \[5, 5\] view"):
        ops.backend_plda_dense(x, 6, *tabs, out=torch.zeros((4, 5), dtype=torch.float32, device=DEV))
    tight = torch.from_numpy(np.array(c["unit"][:5])).to(DEV)      # pitch 6: below d rounded up to 4
    with pytest.raises(XvError, match="score_dense: the pitch must reach d rounded up to 4"):
        ops.score_dense(tight, 6)
    with pytest.raises(XvError, match="backend_plda_dense: the pitch must reach d rounded up to 4"):
        ops.backend_plda_dense(tight, 6, *tabs)
    two = tuple(torch.from_numpy(np.concatenate([t, t])).to(DEV) for t in (c["coef"], c["k0"]))
    with pytest.raises(ValueError, match="the single entry of one utterance"):
        ops.backend_plda_dense(x, 6, two[0], tabs[1], two[1])
    with pytest.raises(XvError, match="x and out overlap"):
        ops.score_dense(x, 6, out=x[:, :5])
    assert tuple(ops.score_dense(x, 6).shape) == (5, 5)      # and the device still works afterwards
