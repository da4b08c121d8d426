"""Cohort statistics of PLDA scores and the AS-norm of scores on the device, on a real MI355X: xv_backend_plda_cohort_stats and
xv_score_normalize through ops.py against fp64 arithmetic on the SAME fp32 tables - the unfactored log-likelihood ratio of
backend_ref.trials_from_tables, a full sort where the kernel selects - and the tables against the closed form (backend_adapt_ref.dense_llr).

Tolerance (EPS = 2^-24, kd = d rounded up to 4, chain(d) = 4 * ceil(d / 256) + 6; the budget is stated in csrc/xv_backend_cohort.hip): the
kernel's element v(r, j) = (slab + C_q[j]) + R[r] is off by at most
    delta(r, j) = c1 * EPS * (sum_c |xs_c t_c| + sum |terms of C_q| + sum |terms of R| + |k0|),    c1 = max(2 kd + 2, chain(d) + 3) + 4
- the GEMM's kd steps in whatever order (a product and an add each: two roundings a step, two more inside xs), chain(d) adds and the roundings
inside a term for the two row sums, then for every part the fma that ends R and the two final adds (+ 3) and the second order (+ 1: c1 EPS is
below 1e-4).  No further factor: this c1 is the whole of c.  The mean of
the k largest is 1-Lipschitz in the sup norm of the row, the deviation 2-Lipschitz (sorted values move by at most delta each, the centred
ones by twice that), so |d mu| <= max_j delta + EPS |mu| and |d sigma| <= 2 max_j delta + EPS |sigma| (the final rounding to fp32).
profiles/plda_cohort_bounds.txt records the worst observed share of these bounds."""
import numpy as np
import pytest

from tests import backend_adapt_ref as A
from tests import backend_ref as R

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
DEV = "cuda:0"
COUNTS = np.array([1, 3, 8])
ROWS, N_MAX = 130, 1031


def _ops():
    import torch
    from tf_kaldi_speaker_amd import ops
    return torch, ops


def _c1(d):
    """The roundings of one element v(r, j), from the add chains stated in csrc/xv_backend_cohort.hip."""
    return max(2 * ((d + 3) // 4 * 4) + 2, R.chain(d) + 3) + 4


def _dev(torch, a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def _prepared(torch, a):
    """A prepared-layout device matrix: pitch = d rounded up to 4, zero padding."""
    rows, d = a.shape
    buf = torch.zeros((rows, (d + 3) // 4 * 4), dtype=torch.float32, device=DEV)
    buf[:, :d] = _dev(torch, a)
    return buf


def _designed(rs, rows, n, d, psi):
    """Model rows x near one vector e0 (drawn at the scale of a PLDA-normalised row) and a cohort of one-utterance-like random rows whose
    first eight are beta * a e0 + noise, beta = 1, 0.88, ...: the ratio rises with beta on [0, 1], so every row's top scores are those eight,
    well apart - the deviation of any top-k >= 2 is far above 1 % of the row's score range (checked on the reference in _check)."""
    e0 = rs.randn(d) * np.sqrt(psi + 0.3)
    x = e0 + 0.05 * rs.randn(rows, d)
    c = rs.randn(n, d) * np.sqrt(psi + 1.0) * 0.35
    a1 = psi / (psi + 1.0)
    for j in range(min(n, 8)):
        c[j] = (1.0 - 0.12 * j) * a1 * e0 + 0.02 * rs.randn(d)
    return x.astype(np.float32), c.astype(np.float32)


class _Case(object):
    """Inputs of one (d, n_distinct), the fp64 scores of the full 130 x 1031 problem from the fp32 tables, and delta; built once, read only."""

    def __init__(self, d, n_distinct):
        from tf_kaldi_speaker_amd.misc import backend as B
        rs = np.random.RandomState(100 * d + n_distinct)
        self.d, self.kd = d, (d + 3) // 4 * 4
        self.psi = np.sort(rs.uniform(0.05, 5.0, d))[::-1].copy()
        self.counts = COUNTS[:n_distinct]
        self.nidx = (np.arange(ROWS) % n_distinct).astype(np.int64)
        self.x, self.c = _designed(rs, ROWS, N_MAX, d, self.psi)
        self.coef, self.g, self.k0 = B.plda_coefficients(self.psi, self.counts)
        tj = np.arange(N_MAX)
        out = [R.trials_from_tables(self.x[r:r + 1], self.c, np.zeros_like(tj), tj, self.nidx[r:r + 1], self.coef, self.g, self.k0, d) for r in range(ROWS)]
        self.scores = np.stack([o[0] for o in out])
        # the |terms| of the factored form, from the same tables in double
        a, iv, g = (t.astype(np.float64)[..., :d] for t in (self.coef[:, 0], self.coef[:, 1], self.g))
        x64, c64, q = self.x.astype(np.float64), self.c.astype(np.float64), self.nidx
        gemm = np.abs(iv[q] * a[q] * x64) @ np.abs(c64).T
        cterm = (0.5 * np.abs(g[None, :] - iv)[:, None, :] * (c64 * c64)[None, :, :]).sum(axis=2)
        rterm = (0.5 * iv[q] * a[q] ** 2 * x64 * x64).sum(axis=1)
        self.terms = gemm + cterm[q] + rterm[:, None] + np.abs(self.k0.astype(np.float64))[q][:, None]
        self.delta = _c1(d) * EPS * self.terms
        for arr in (self.scores, self.terms, self.delta):
            arr.setflags(write=False)

    def device(self, torch, rows, n):
        return (_prepared(torch, self.x[:rows]), _prepared(torch, self.c[:n]), self.nidx[:rows]) + tuple(_dev(torch, t) for t in (self.coef, self.g, self.k0))


_CASES = {}


def _case(d, n_distinct):
    if (d, n_distinct) not in _CASES:
        _CASES[(d, n_distinct)] = _Case(d, n_distinct)
    return _CASES[(d, n_distinct)]


def _check(got, scores, delta, top_k, floor=True):
    """got [rows, 2] against the full sort of `scores` within the bound from `delta`; -> the worst share of the bound."""
    got = got.astype(np.float64)
    ref = A.top_k_stats(scores, top_k)
    k = min(top_k, scores.shape[1])
    assert got.shape == ref.shape and np.all(np.isfinite(got))
    if k == 1:
        assert np.all(ref[:, 1] == 1e-6) and np.all(got[:, 1] == np.float32(1e-6))
    elif floor:      # the design holds: a degenerate input cannot hide an error
        assert np.all(ref[:, 1] >= 0.01 * (scores.max(axis=1) - scores.min(axis=1))), float((ref[:, 1] / (scores.max(axis=1) - scores.min(axis=1))).min())
    dmax = delta.max(axis=1)
    tol_mu, tol_sd = dmax + EPS * np.abs(ref[:, 0]), 2 * dmax + EPS * np.abs(ref[:, 1])
    e_mu, e_sd = np.abs(got[:, 0] - ref[:, 0]), np.abs(got[:, 1] - ref[:, 1])
    share = max(float((e_mu / tol_mu).max()), float((e_sd / tol_sd).max()))
    assert np.all(e_mu <= tol_mu) and np.all(e_sd <= tol_sd), (top_k, share)
    return share


def _stats(ops, dev, d, top_k, **kw):
    x, c, nidx, coef, g, k0 = dev
    return ops.backend_plda_cohort_stats(x, c, d, nidx, coef, g, k0, top_k, **kw)


@pytest.mark.parametrize("n_distinct", [1, 3])
@pytest.mark.parametrize("rows", [1, 130])
@pytest.mark.parametrize("n_cohort", [1, 5, 255, 256, 257, 1031])
@pytest.mark.parametrize("d", [30, 200, 601])
def test_cohort_stats(d, n_cohort, rows, n_distinct):
    torch, ops = _ops()
    case = _case(d, n_distinct)
    dev = case.device(torch, rows, n_cohort)
    worst = 0.0
    for top_k in sorted({1, 2, n_cohort - 1, n_cohort, n_cohort + 7}):
        if top_k <= 0:
            continue                                        # (n_cohort = 1: top_k = 0 is a refusal, test_refusals)
        got = _stats(ops, dev, d, top_k).cpu().numpy()
        worst = max(worst, _check(got, case.scores[:rows, :n_cohort], case.delta[:rows, :n_cohort], top_k))
    print("plda cohort d=%d n=%d rows=%d counts=%d: worst error / bound %.4f" % (d, n_cohort, rows, n_distinct, worst))


def test_null_nidx_is_entry_zero_and_the_tables_are_the_closed_form():
    torch, ops = _ops()
    case = _case(30, 3)
    x, c, _, coef, g, k0 = case.device(torch, ROWS, 257)
    got = ops.backend_plda_cohort_stats(x, c, 30, None, coef, g, k0, 20)
    want = ops.backend_plda_cohort_stats(x, c, 30, np.zeros(ROWS, np.int64), coef, g, k0, 20)
    assert torch.equal(got, want)
    # the scores the tolerance is taken against are the restatement's closed form, up to the rounding of the tables
    full = A.dense_llr(case.x[:9], case.c[:257], case.psi, case.counts[case.nidx[:9]])
    assert np.all(np.abs(full - case.scores[:9, :257]) <= 1e-5 * case.terms[:9, :257])


def test_two_row_tiles_from_a_one_tile_workspace():
    """130 rows through a workspace of exactly one 128-row tile: two fold + GEMM + select rounds.  The workspace is, in floats,
    [n_distinct][P] column terms + tile * (P slab + K operand + 1 row term), P = n_cohort and K = d rounded up to 4."""
    torch, ops = _ops()
    for d in (30, 200):
        case = _case(d, 3)
        one_tile = ops.backend_plda_cohort_workspace_bytes(128, 257, d, 3)
        assert one_tile == (3 * 260 + 128 * (260 + case.kd + 1)) * 4
        assert ops.backend_plda_cohort_workspace_bytes(130, 257, d, 3) == (3 * 260 + 256 * (260 + case.kd + 1)) * 4
        dev = case.device(torch, ROWS, 257)
        got = _stats(ops, dev, d, 20, ws_bytes=one_tile)
        _check(got.cpu().numpy(), case.scores[:, :257], case.delta[:, :257], 20)
        assert torch.equal(got, _stats(ops, dev, d, 20))     # the same bits from one round


def _dense(case_like, x, c, nidx):
    coef, g, k0, d = case_like
    tj = np.arange(len(c))
    return np.stack([R.trials_from_tables(x[r:r + 1], c, np.zeros_like(tj), tj, nidx[r:r + 1], coef, g, k0, d)[0] for r in range(len(x))])


def test_ties_negative_scores_and_identical_rows():
    torch, ops = _ops()
    case = _case(30, 3)
    d = 30
    tabs = (case.coef, case.g, case.k0, d)
    dtabs = tuple(_dev(torch, t) for t in (case.coef, case.g, case.k0))
    # every cohort row four times: top_k = 6 takes the best run whole and cuts the second one in half
    c = np.repeat(case.c[:10], 4, axis=0)
    s = _dense(tabs, case.x, c, case.nidx)
    top = -np.sort(-s, axis=1)
    assert np.all(top[:, 3] > top[:, 4]) and np.all(top[:, 4] == top[:, 7])      # the cut (after 6) falls inside a run of equal scores
    delta = np.repeat(case.delta[:, :10], 4, axis=1)
    got = ops.backend_plda_cohort_stats(_prepared(torch, case.x), _prepared(torch, c), d, case.nidx, *dtabs, top_k=6)
    _check(got.cpu().numpy(), s, delta, 6)
    # every score negative: a cohort far from every model row
    cn = (-8.0 * case.c[8:108]).astype(np.float32)
    sn = _dense(tabs, case.x[:3], cn, case.nidx[:3])
    assert sn.max() < -1.0
    a, iv, g = (t.astype(np.float64)[..., :d] for t in (case.coef[:, 0], case.coef[:, 1], case.g))
    q = case.nidx[:3]
    x64, c64 = case.x[:3].astype(np.float64), cn.astype(np.float64)
    terms = np.abs(iv[q] * a[q] * x64) @ np.abs(c64).T + (0.5 * np.abs(g[None, :] - iv)[:, None, :] * (c64 * c64)[None, :, :]).sum(axis=2)[q] \
        + (0.5 * iv[q] * a[q] ** 2 * x64 * x64).sum(axis=1)[:, None] + np.abs(case.k0.astype(np.float64))[q][:, None]
    dn = _c1(d) * EPS * terms
    got = ops.backend_plda_cohort_stats(_prepared(torch, case.x[:3]), _prepared(torch, cn), d, q, *dtabs, top_k=10)
    _check(got.cpu().numpy(), sn, dn, 10, floor=False)
    # identical model rows (one count): identical statistics, bit for bit
    xi = np.repeat(case.x[5:6], 130, axis=0)
    got = ops.backend_plda_cohort_stats(_prepared(torch, xi), _prepared(torch, case.c[:257]), d, np.full(130, 2), *dtabs, top_k=20).cpu().numpy()
    assert np.all(got.view(np.int32) == got[0].view(np.int32))


def test_score_normalize_is_score_trials_bit_for_bit():
    """Cosine inputs through both: score_trials with statistics against score_trials without, then score_normalize."""
    torch, ops = _ops()
    rs = np.random.RandomState(11)
    unit = lambda v: v / np.linalg.norm(v, axis=1, keepdims=True)
    e, t = _prepared(torch, unit(rs.randn(7, 64))), _prepared(torch, unit(rs.randn(5, 64)))
    e_stats = _dev(torch, np.stack([rs.uniform(-0.1, 0.2, 7), rs.uniform(0.05, 0.2, 7)], axis=1))
    t_stats = _dev(torch, np.stack([rs.uniform(-0.1, 0.2, 5), rs.uniform(0.05, 0.2, 5)], axis=1))
    for m in (1, 255, 256, 257, 1000):
        ei, ti = rs.randint(0, 7, m), rs.randint(0, 5, m)
        want = ops.score_trials(e, t, 64, ei, ti, e_stats, t_stats)
        raw = ops.score_trials(e, t, 64, ei, ti)
        got = ops.score_normalize(raw, ei, ti, e_stats, t_stats)
        assert got.data_ptr() != raw.data_ptr() and torch.equal(got, want)
        same = ops.score_normalize(raw, ei, ti, e_stats, t_stats, out=raw)      # in place
        assert same.data_ptr() == raw.data_ptr() and torch.equal(raw, want)
    with pytest.raises(IndexError, match="ei holds a value outside 0 .. 6"):
        ops.score_normalize(raw, np.full(1000, 7), ti, e_stats, t_stats)
    with pytest.raises(IndexError, match="ti holds a value outside 0 .. 4"):
        ops.score_normalize(raw, ei, np.full(1000, -1), e_stats, t_stats)
    from tf_kaldi_speaker_amd._lib import XvError
    buf = torch.zeros(1001, dtype=torch.float32, device=DEV)
    with pytest.raises(XvError, match="scores and out overlap"):
        ops.score_normalize(buf[:1000], ei, ti, e_stats, t_stats, out=buf[1:])


def test_two_calls_are_bit_identical_and_the_workspace_is_not_read():
    torch, ops = _ops()
    from tf_kaldi_speaker_amd import _lib
    from tf_kaldi_speaker_amd._host import _p, _s
    import ctypes as C
    case = _case(200, 3)
    dev = case.device(torch, ROWS, N_MAX)
    first = _stats(ops, dev, 200, 300)
    assert torch.equal(first, _stats(ops, dev, 200, 300))
    # a workspace full of 1e30 in front of the call: nothing of it may reach a result
    x, c, nidx, coef, g, k0 = dev
    ws_bytes = ops.backend_plda_cohort_workspace_bytes(128, N_MAX, 200, 3)      # one tile: the second round runs over the first one's leftovers
    ws = torch.full((ws_bytes // 4,), 1e30, dtype=torch.float32, device=DEV)
    stats = torch.empty((ROWS, 2), dtype=torch.float32, device=DEV)
    nidx_d = _dev(torch, nidx, np.int32)
    _lib.call("xv_backend_plda_cohort_stats", _s(), _p(x), x.stride(0), ROWS, _p(nidx_d), _p(c), c.stride(0), N_MAX, 200, _p(coef), coef.shape[2], 3,
              _p(g), _p(k0), 300, _p(stats), _p(ws), C.c_size_t(ws_bytes))
    assert torch.equal(stats, first)


def test_refusals():
    """Every refusal comes back by name, before anything is launched."""
    torch, ops = _ops()
    import ctypes as C
    from tf_kaldi_speaker_amd import _lib
    from tf_kaldi_speaker_amd._host import _p, _s
    from tf_kaldi_speaker_amd._lib import XvError
    case = _case(30, 3)
    x, c, nidx, coef, g, k0 = case.device(torch, 4, 5)
    call = lambda **kw: ops.backend_plda_cohort_stats(kw.get("x", x), kw.get("c", c), 30, kw.get("nidx", nidx), coef, g, k0, kw.get("top_k", 2),
                                                      ws_bytes=kw.get("ws_bytes"))
    with pytest.raises(XvError, match="top_k must be positive"):
        call(top_k=0)
    with pytest.raises(XvError, match="n_cohort must be positive"):
        call(c=c[:0])
    need = ops.backend_plda_cohort_workspace_bytes(128, 5, 30, 3)
    assert need == (3 * 8 + 128 * (8 + 32 + 1)) * 4
    with pytest.raises(XvError, match="at least one 128-row tile"):
        call(ws_bytes=need - 4)
    with pytest.raises(XvError, match="both pitches must reach d rounded up to 4"):
        call(x=_dev(torch, case.x[:4]))                     # pitch 30
    with pytest.raises(IndexError, match="nidx holds a value outside 0 .. 2"):
        call(nidx=np.array([0, 1, 2, 3]))
    with pytest.raises(ValueError, match="one entry per row"):
        call(nidx=np.array([0, 1]))
    flat = torch.zeros(4 * 32 + 1, dtype=torch.float32, device=DEV)
    with pytest.raises(XvError, match="the cohort must be a GEMM operand"):
        call(c=flat[1:].view(4, 32))                        # base off the 16-byte grid
    with pytest.raises(XvError, match="the cohort must be a GEMM operand"):
        call(c=torch.zeros((4, 34), dtype=torch.float32, device=DEV))
    ws = torch.zeros(need // 4 + 1, dtype=torch.float32, device=DEV)
    stats = torch.empty((4, 2), dtype=torch.float32, device=DEV)
    with pytest.raises(XvError, match="16-byte aligned"):   # a workspace base off the 16-byte grid
        _lib.call("xv_backend_plda_cohort_stats", _s(), _p(x), 32, 4, _p(None), _p(c), 32, 5, 30, _p(coef), 32, 3, _p(g), _p(k0), 2, _p(stats),
                  C.c_void_p(ws.data_ptr() + 4), C.c_size_t(need))
    got = call()                                            # and the device still works afterwards
    assert got.shape == (4, 2) and np.isfinite(got.cpu().numpy()).all()
