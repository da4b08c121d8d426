"""xv_backend_pca_plda on a real MI355X through ops.backend_pca_plda, against the fp64 restatement tests/pca_plda_ref.py on the same fp32
rows: the kept dimension exactly, the eigenvalues against numpy.linalg.eigh, the fp32 map against the two identities that define it, the
tables, the bits (a second call, another slot of the batch, another pitch), what is left untouched, and the final scores of
op -> backend_affine -> backend_plda_normalize -> backend_plda_dense.

Tolerances (EPS = 2^-24, E64 = 2^-52).
  p                  exact: every case meets the decision-gap conditions (tests/test_pca_plda_ref.py).
  s, psi             nobody had measured a fp64 Jacobi on this device: the worst |got - eigh| / largest over the shapes here was measured
                     (profiles/pca_plda_bounds.txt: s 2.2e-15, psi 2.6e-14, both at D = 256, n = 2048) and 8 times that is asserted - the
                     margin tests/test_vbx_ref.py uses for the same reason.
  A W A^T / D = I    A32 = A (1 + delta), |delta| <= EPS per element: |A32 W A32^T - A W A^T| <= (2 EPS + EPS^2) |A32| |W| |A32|^T, plus the
  A B A^T / D = psi  defect of the double solve, at most 8 p E64 cond(W') (Cholesky and triangular inverse: backward stable) - times psi_1 for B.
  tables             one fp32 rounding of the double value, plus the propagated error of psi: every table entry has |d / d psi| <= 1
                     (k0: <= p), so PSI_TOL * psi_1 (* p) is added.
  scores             the existing dense_tol construction of tests/test_gpu_dense_scores.py on the recording's own fp32 tables and prepared
                     rows; plus, derived below in _score_bound, the rounding of A and the offset and the fp32 affine map and normalisation
                     propagated to first and second order through the score; plus the rounding of the tables; plus the subspace term
                     E64 (sweeps / gap + 8 p cond(W')) sum|terms|, negligible under the gap condition."""
import ctypes as C

import numpy as np
import pytest

from tests import backend_ref as R
from tests import pca_plda_ref as P

pytestmark = pytest.mark.gpu

EPS, E64 = 2.0 ** -24, 2.0 ** -52
DEV = "cuda:0"
S_TOL = 8 * 2.2e-15        # |s - eigh| / s_1
PSI_TOL = 8 * 2.6e-14      # |psi - eigh| / psi_1
ALL = [(d, n, t) for d, n, targets in P.SHAPES for t in targets]
E2E_ROWS = 96              # the rows of a recording whose scores are compared (all of them below that)


def _ops():
    import torch
    from tf_kaldi_speaker_amd import ops
    return torch, ops


def _p4(d):
    return (d + 3) // 4 * 4


def _pack(xs, ld, gap=0, fill=np.nan):
    """The recordings back to back on the pitch ld, `gap` floats in front of each: (host buffer filled with `fill` outside the rows, offsets, n)."""
    d = xs[0].shape[1]
    n = np.asarray([x.shape[0] for x in xs], np.int64)
    offsets = np.concatenate([[0], np.cumsum(n * ld + gap)])[:-1] + gap
    host = np.full(int((n * ld + gap).sum()) + gap, fill, np.float32)
    for x, o, r in zip(xs, offsets, n):
        host[o:o + r * ld].reshape(r, ld)[:, :d] = x
    return host, offsets, n


_MODELS = {}


def _model(c):
    """(W, B, mu) of a case on the device, uploaded once."""
    import torch
    d = c["w"].shape[0]
    if d not in _MODELS:
        _MODELS[d] = tuple(torch.from_numpy(np.array(c[k])).to(DEV) for k in ("w", "b", "mu"))
    return _MODELS[d]


def _call(xs, c, target, ld=None, gap=0, fill=np.nan):
    torch, ops = _ops()
    d = xs[0].shape[1]
    ld = d if ld is None else ld
    host, offsets, n = _pack(xs, ld, gap, fill)
    x = torch.from_numpy(host).to(DEV)
    got = ops.backend_pca_plda(x, offsets, n, d, *_model(c), target=target, ld=np.full(n.size, ld, np.int64))
    return got, x, offsets


def _host(got):
    return {k: v.cpu().numpy() for k, v in got.items()}


def _same_bits(a, b, j=0, k=0):
    """Recording j of a and recording k of b hold the same bits in every output (NaN patterns included)."""
    return all(np.array_equal(a[key][j].view(np.int32 if a[key].dtype.itemsize == 4 else np.int64),
                              b[key][k].view(np.int32 if b[key].dtype.itemsize == 4 else np.int64)) for key in a)


_REFS = {}


def _ref(d, n, target, seed=0):
    key = (d, n, target, seed)
    if key not in _REFS:
        c = P.case(d, n, seed)
        _REFS[key] = P.estimate(c["x"], c["w"], c["b"], c["mu"], target)
    return _REFS[key]


def _check_model(g, j, c, ref, d, tag):
    """Recording j of the host outputs g against the reference model ref: p, s, psi, the two identities, the tables, the padding.
    -> (s error, psi error) relative to the largest."""
    from tf_kaldi_speaker_amd.misc import backend as B
    p, d4 = int(g["p"][j]), _p4(d)
    assert p == ref["p"], (tag, p, ref["p"])
    s_err = float(np.abs(g["s"][j] - ref["s"]).max() / ref["s"][0])
    psi_err = float(np.abs(g["psi64"][j][:p] - ref["psi"]).max() / ref["psi"][0])
    a32 = g["a"][j][:p, :d].astype(np.float64)
    cond = np.linalg.cond(ref["wp"])
    absa = np.abs(a32)
    tol_w = (2 * EPS + EPS * EPS) * (absa @ np.abs(c["w"]) @ absa.T) / d + 8 * p * E64 * cond
    tol_b = (2 * EPS + EPS * EPS) * (absa @ np.abs(c["b"]) @ absa.T) / d + 8 * p * E64 * cond * ref["psi"][0]
    err_w = np.abs(a32 @ c["w"] @ a32.T / d - np.eye(p))
    err_b = np.abs(a32 @ c["b"] @ a32.T / d - np.diag(g["psi64"][j][:p]))
    print("%s: p=%d sweeps=%s  s error %.3e  psi error %.3e (of the largest)  A W A^T / D - I: worst / bound %.3f  A B A^T / D - psi: %.3f"
          % (tag, p, g["sweeps"][j].tolist(), s_err, psi_err, float((err_w / tol_w).max()), float((err_b / tol_b).max())))
    assert s_err <= S_TOL and psi_err <= PSI_TOL, (tag, s_err, psi_err)
    assert np.all(np.diff(g["s"][j]) <= 0) and g["s"][j][-1] >= 0 and np.all(np.diff(g["psi64"][j][:p]) <= 0) and g["psi64"][j][p - 1] >= 0
    assert np.all(err_w <= tol_w) and np.all(err_b <= tol_b), tag
    # the offset is -T' mu' = -(A mu) / sqrt(D): an identity between two outputs, each rounded once (free of an eigenvector's sign)
    off = -(a32 @ c["mu"]) / np.sqrt(d)
    assert np.all(np.abs(g["offset"][j][:p] - off) <= EPS * np.abs(off) + (EPS + 8 * d * E64) * (absa @ np.abs(c["mu"])) / np.sqrt(d)), tag
    # the tables: one fp32 rounding of the double values of the reference's psi, plus psi's own error through derivatives <= 1
    a64, iv64, g64, k064 = R.coefficients(ref["psi"], [1])
    dpsi = PSI_TOL * ref["psi"][0]
    for name, got, want in (("psi", g["psi"][j][:p], ref["psi"]), ("a", g["coef"][j][0][:p], a64[0]), ("iv", g["coef"][j][1][:p], iv64[0]), ("g", g["g"][j][:p], g64)):
        assert np.all(np.abs(got.astype(np.float64) - want) <= EPS * np.abs(want) + dpsi), (tag, name)
    assert abs(float(g["k0"][j]) - k064[0]) <= EPS * abs(k064[0]) + p * dpsi, tag
    # ... and they are plda_coefficients of the device's own psi, to the last bit but for the two logarithms of k0
    coef, gt, k0 = B.plda_coefficients(g["psi64"][j][:p], [1])
    assert np.array_equal(coef[0, :, :p], g["coef"][j][:, :p]) and np.array_equal(gt[:p], g["g"][j][:p]) and abs(float(k0[0]) - float(g["k0"][j])) <= 2 * EPS * abs(float(k0[0]))
    assert np.array_equal(g["psi"][j][:p], g["psi64"][j][:p].astype(np.float32))
    # the padding: zero behind p rows / d columns of the map and behind p in every vector; psi64 behind p untouched
    assert np.all(g["a"][j][p:] == 0) and np.all(g["a"][j][:, d:] == 0) and g["a"][j].shape == (d4, d4)
    for key in ("offset", "psi", "g"):
        assert np.all(g[key][j][p:] == 0), (tag, key)
    assert np.all(g["coef"][j][:, p:] == 0) and np.all(np.isnan(g["psi64"][j][p:])) and np.all(np.isfinite(g["a"][j]))
    return s_err, psi_err


def _score_bound(x, a32, off32, psi_ref, y32, coef32, g32, k032, p, d, sweeps, sgap, cond):
    """The bound of |device score - fp64 restatement| for rows x (fp32 values in double), derived:
    (1) u = A x + offset.  The device's A32 and offset32 are its double values rounded once: |du| <= EPS (|A32| |x| + |off32|) (1 + 2 EPS);
        the fp32 GEMM over kd = d rounded up to 4 steps rounds at most twice a step, the bias add once: (2 kd + 3) EPS (|A32| |x| + |off32|).
    (2) y = u sqrt(p / q), q = sum_c u_c^2 / (psi_c + 1): dq <= sum_c (2 |u_c| du_c + du_c^2) / (psi_c + 1) + EPS q (psi rounded to fp32), so
        dy_c <= 1.01 (r du_c + |y_c| dq / (2 q)) (1 % for the second order of the square root), plus the kernel's own tolerance
        2 (chain(p) + 2) EPS p per element (tests/test_gpu_backend.py).
    (3) through the score sum_c -0.5 iv (t - a e)^2 + 0.5 g t^2 + k0 with first and second order kept:
        iv |t - a e| (dt + a de) + 0.5 iv (dt + a de)^2 + g |t| dt + 0.5 g dt^2.
    (4) the tables: each entry rounded once, psi's own error PSI_TOL psi_1 through derivatives <= 1.
    (5) dense_tol of tests/test_gpu_dense_scores.py on the device's own rows and tables.
    (6) the double part: E64 (sweeps / gap + 8 p cond(W')) sum|terms|."""
    kd, kp = _p4(d), _p4(p)
    absu = np.abs(x) @ np.abs(a32).T + np.abs(off32)[None, :]
    u = x @ a32.T + off32[None, :]
    du = (EPS * (1 + 2 * EPS) + (2 * kd + 3) * EPS) * absu
    w = 1.0 / (psi_ref + 1.0)
    q = (u * u * w).sum(axis=1, keepdims=True)
    r = np.sqrt(p / q)
    dq = ((2 * np.abs(u) * du + du * du) * w).sum(axis=1, keepdims=True) + EPS * q
    y = u * r
    dy = 1.01 * (r * du + np.abs(y) * dq / (2 * q)) + 2 * (R.chain(p) + 2) * EPS * p
    a, iv, g = (t.astype(np.float64)[:p] for t in (coef32[0], coef32[1], g32))
    k0 = float(k032)
    e, t = y[:, None, :], y[None, :, :]
    de, dt = dy[:, None, :], dy[None, :, :]
    diff = np.abs(t - a * e)
    dd = dt + a * de
    prop = (iv * diff * dd + 0.5 * iv * dd * dd + g * np.abs(t) * dt + 0.5 * g * dt * dt).sum(axis=2)
    dpsi = PSI_TOL * psi_ref[0]
    terms = (0.5 * iv * diff * diff + 0.5 * g * t * t).sum(axis=2) + abs(k0)
    tables = ((0.5 * (EPS * iv + dpsi)) * diff * diff + iv * diff * (EPS * a + dpsi) * np.abs(e) + 0.5 * (EPS * g + dpsi) * t * t).sum(axis=2) + EPS * abs(k0) + p * dpsi
    y64 = y32.astype(np.float64)[:, :p]
    gemm = np.abs(iv * a * y64) @ np.abs(y64).T
    cterm = (0.5 * np.abs(g - iv) * (y64 * y64)).sum(axis=1)
    rterm = (0.5 * iv * a ** 2 * y64 * y64).sum(axis=1)
    c1 = max(2 * kp + 2, R.chain(p) + 3) + 4
    dense = c1 * EPS * (gemm + cterm[None, :] + rterm[:, None] + abs(k0))
    double = E64 * (sweeps / min(sgap, 1.0) + 8 * p * cond) * terms
    return dense + prop + tables + double, (dense, prop, tables, double)


def _check_scores(got, j, rows_dev, x, c, ref, d, target, tag):
    """The device pipeline on the rows rows_dev ([n, d4] zero-padded, the same fp32 values as x) with recording j's outputs, against the
    restatement's scores of those rows."""
    torch, ops = _ops()
    p = int(got["p"][j])
    p4 = _p4(p)
    u = ops.backend_affine(rows_dev, got["a"][j, :p4], got["offset"][j, :p4])
    y = ops.backend_plda_normalize(u, p, got["psi"][j, :p], out=u)
    s = ops.backend_plda_dense(y, p, got["coef"][j:j + 1], got["g"][j], got["k0"][j:j + 1]).cpu().numpy().astype(np.float64)
    x64 = x.astype(np.float64)
    want = P.scores_from(x64, ref["a"], ref["offset"], ref["psi"])
    g = {k: v[j].cpu().numpy() for k, v in got.items()}
    sgap = P.decision_gaps(c["x"], target)[1]
    bound, parts = _score_bound(x64, g["a"][:p, :d].astype(np.float64), g["offset"][:p].astype(np.float64), ref["psi"], y.cpu().numpy(), g["coef"],
                                g["g"], g["k0"], p, d, float(g["sweeps"].max()), sgap, np.linalg.cond(ref["wp"]))
    err = np.abs(s - want)
    at = np.unravel_index(np.argmax(err / bound), err.shape)
    print("%s: scores of size %.3g: worst error %.3e, worst error / bound %.4f (there: dense %.2e, map and normalisation %.2e, tables %.2e, double %.2e)"
          % (tag, np.abs(want).max(), err.max(), float((err / bound).max()), parts[0][at], parts[1][at], parts[2][at], parts[3][at]))
    assert np.all(err <= bound), tag


@pytest.mark.parametrize("d,n,target", ALL)
def test_model_and_scores(d, n, target):
    torch, ops = _ops()
    c, ref = P.case(d, n), _ref(d, n, target)
    tag = "pca_plda D=%d n=%d target=%g" % (d, n, target)
    got, x, offsets = _call([c["x"]], c, target, ld=_p4(d), fill=0.0)      # the zero-padded pitch of the chain: the rows feed backend_affine below
    g = _host(got)
    _check_model(g, 0, c, ref, d, tag)
    again = _host(_call([c["x"]], c, target, ld=_p4(d), fill=0.0)[0])
    assert _same_bits(g, again)                                            # a second call: the same bits
    odd = _host(_call([c["x"]], c, target, ld=d + 3, gap=5)[0])            # another pitch and start, NaN in every float that is not a row's
    assert _same_bits(g, odd)
    _check_scores(got, 0, x.view(n, _p4(d)), c["x"], c, ref, d, target, tag)


def test_both_caps_in_a_batch_of_two():
    """D = 256 and n = 2048 at once, two recordings: the first eigenproblem in the workspace, the second (p = 119 and 122 > 90) too."""
    torch, ops = _ops()
    d, n, target = P.BIG
    cases = [P.case(d, n, seed) for seed in (0, 1)]
    assert all(P.qualifies(c["x"], target) for c in cases)
    got, x, offsets = _call([c["x"] for c in cases], cases[0], target, fill=0.0)
    g = _host(got)
    for j, c in enumerate(cases):
        ref = _ref(d, n, target, seed=j)
        tag = "pca_plda D=%d n=%d target=%g recording %d of 2" % (d, n, target, j)
        assert _check_model(g, j, c, ref, d, tag) is not None and ref["p"] > 90
        rows = x[int(offsets[j]):int(offsets[j]) + E2E_ROWS * d].view(E2E_ROWS, d)
        _check_scores(got, j, rows, c["x"][:E2E_ROWS], c, ref, d, target, tag)
    alone = _host(_call([cases[1]["x"]], cases[0], target, fill=0.0)[0])
    assert _same_bits(g, alone, 1, 0)                                      # the second of two == alone


def test_mixed_batch_slots_and_pitches():
    """n = 1, 3, 40 and 300 in one call at D = 36: p = 0 for the single row (nothing but p and s written), every other recording the
    reference's p and the same bits wherever it sits in the batch and whatever the pitch (36: on the 16-byte grid, 37 and 39: off it)."""
    d, target = 36, 0.5
    c = P.case(d, 40)
    xs = [P.recording(seed, d, n) for seed, n in ((0, 1), (1, 3), (0, 40), (2, 300))]
    assert all(P.qualifies(x, target) for x in xs[1:])
    g = _host(_call(xs, c, target, ld=36)[0])
    assert g["p"].tolist() == [0] + [P.estimate(x, c["w"], c["b"], c["mu"], target)["p"] for x in xs[1:]]
    for j in (1, 2, 3):
        ref = P.estimate(xs[j], c["w"], c["b"], c["mu"], target)
        _check_model(g, j, c, ref, d, "pca_plda mixed batch recording %d (n=%d)" % (j, xs[j].shape[0]))
    # p = 0: s (all zero for a single row) and the sweeps of the first eigenproblem; everything else as the wrapper allocated it
    assert np.all(g["s"][0] == 0) and g["sweeps"][0].tolist() == [1, 0]
    assert all(np.all(np.isnan(g[k][0])) for k in ("a", "offset", "psi", "coef", "g", "k0", "psi64"))
    order = [3, 0, 2, 1]
    for ld, gap in ((37, 0), (39, 3), (36, 4)):
        moved = _host(_call([xs[i] for i in order], c, target, ld=ld, gap=gap)[0])
        for slot, i in enumerate(order):
            assert _same_bits(g, moved, i, slot), (ld, gap, i)
    equal = _host(_call([np.repeat(xs[2][:1], 5, axis=0), xs[2]], c, target)[0])      # five equal rows: a zero covariance, p = 0
    assert equal["p"].tolist() == [0, int(g["p"][2])] and _same_bits(g, equal, 2, 1)


def test_a_recording_outside_the_buffer_is_skipped_and_flagged():
    """The kernel's own check, behind the wrapper's: device index arrays that would take a recording outside x give p = -1 for it, its
    slots untouched, its neighbours the bits they have alone."""
    torch, ops = _ops()
    from tf_kaldi_speaker_amd import _lib
    from tf_kaldi_speaker_amd._host import _p, _s
    d, target = 36, 0.5
    c = P.case(d, 40)
    xs = [P.recording(seed, d, 40) for seed in (0, 1, 2, 3, 4, 5)]
    host, offsets, n = _pack(xs, d)
    good = _host(_call(xs, c, target)[0])
    x = torch.from_numpy(host).to(DEV)
    ld = np.full(6, d, np.int64)
    bad_off, bad_n, bad_ld = offsets.copy(), n.copy(), ld.copy()
    bad_off[0] = -1                       # starts in front of x
    bad_off[1] = host.size - 40 * d + 1   # the last row ends one float behind x
    bad_n[2] = 2049                       # above the cap
    bad_ld[3] = d - 1                     # a pitch below d
    bad_n[4] = 0
    w, b, mu = _model(c)
    d4 = _p4(d)
    nan32 = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)
    out = dict(p=torch.full((6,), 77, dtype=torch.int32, device=DEV), a=nan32(6, d4, d4), offset=nan32(6, d4), psi=nan32(6, d4), coef=nan32(6, 2, d4),
               g=nan32(6, d4), k0=nan32(6), s=torch.full((6, d), float("nan"), dtype=torch.float64, device=DEV),
               psi64=torch.full((6, d), float("nan"), dtype=torch.float64, device=DEV), sweeps=torch.full((6, 2), -1, dtype=torch.int32, device=DEV))
    ws_bytes = ops.backend_pca_plda_workspace_bytes(6, d)
    ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=DEV)
    up = lambda a, t: torch.from_numpy(np.ascontiguousarray(a, dtype=t)).to(DEV)
    off_d, n_d, ld_d = up(bad_off, np.int64), up(bad_n, np.int32), up(bad_ld, np.int32)      # (named: they must outlive the call)
    _lib.call("xv_backend_pca_plda", _s(), _p(x), C.c_int64(x.numel()), _p(off_d), _p(n_d), _p(ld_d), 6, d, 40,
              C.c_double(target), _p(w), _p(b), _p(mu), _p(out["p"]), _p(out["a"]), _p(out["offset"]), _p(out["psi"]), _p(out["coef"]), _p(out["g"]),
              _p(out["k0"]), _p(out["s"]), _p(out["psi64"]), _p(out["sweeps"]), _p(ws), C.c_size_t(ws_bytes))
    g = _host(out)
    assert g["p"].tolist() == [-1, -1, -1, -1, -1, int(good["p"][5])]
    for j in range(5):
        assert all(np.all(np.isnan(g[k][j])) for k in ("a", "offset", "psi", "coef", "g", "k0", "s", "psi64")) and g["sweeps"][j].tolist() == [-1, -1]
    assert _same_bits(g, good, 5, 5)
    # the wrapper refuses every one of these before the upload
    for kw, exc, what in ((dict(x_offsets=bad_off), IndexError, "backend_pca_plda: a recording's rows lie outside the %d floats of x" % host.size),
                          (dict(n=np.where(np.arange(6) == 2, 2049, n)), ValueError, "backend_pca_plda: recording 2 has 2049 rows, the cap is 2048"),
                          (dict(ld=bad_ld), ValueError, "backend_pca_plda: recording 3: the pitch 35 is below the 36 dimensions"),
                          (dict(n=np.where(np.arange(6) == 4, 0, n)), ValueError, r"backend_pca_plda: recording 4 has no row \(n = 0\)")):
        args = dict(x_offsets=offsets, n=n, ld=ld)
        args.update(kw)
        with pytest.raises(exc, match=what):
            ops.backend_pca_plda(x, args["x_offsets"], args["n"], d, w, b, mu, target, ld=args["ld"])


def test_refusals():
    torch, ops = _ops()
    d = 4
    c = P.case(d, 3)
    w, b, mu = _model(c)
    x = torch.from_numpy(np.array(c["x"]).reshape(-1)).to(DEV)
    call = lambda x=x, off=(0,), n=(3,), d=d, w=w, b=b, mu=mu, target=0.5, ld=None: ops.backend_pca_plda(x, np.asarray(off), np.asarray(n), d, w, b, mu, target, ld=ld)
    for kw, exc, what in ((dict(target=0.0), ValueError, r"backend_pca_plda: target must lie in \(0, 1\] \(got 0.0\)"),
                          (dict(target=1.001), ValueError, r"backend_pca_plda: target must lie in \(0, 1\]"),
                          (dict(target=float("nan")), ValueError, r"backend_pca_plda: target must lie in \(0, 1\]"),
                          (dict(d=0), ValueError, r"backend_pca_plda: d must lie in 1 \.\. 256 \(got 0\)"),
                          (dict(d=257), ValueError, r"backend_pca_plda: d must lie in 1 \.\. 256 \(got 257\)"),
                          (dict(x=x.double()), ValueError, "backend_pca_plda: x must be a non-empty contiguous 1-D float32 tensor"),
                          (dict(x=x.view(3, 4)), ValueError, "backend_pca_plda: x must be a non-empty contiguous 1-D float32 tensor"),
                          (dict(n=()), ValueError, "backend_pca_plda: n must be a non-empty 1-D integer array"),
                          (dict(n=(3.0,)), ValueError, "backend_pca_plda: n must be a non-empty 1-D integer array"),
                          (dict(off=(0, 0)), ValueError, "backend_pca_plda: x_offsets must be a 1-D integer array of 1"),
                          (dict(ld=(3,)), ValueError, "backend_pca_plda: recording 0: the pitch 3 is below the 4 dimensions"),
                          (dict(off=(1,)), IndexError, "backend_pca_plda: a recording's rows lie outside the 12 floats of x"),
                          (dict(n=(4,)), IndexError, "backend_pca_plda: a recording's rows lie outside the 12 floats of x"),
                          (dict(w=w.float()), ValueError, r"backend_pca_plda: w must be a contiguous float64 \[4, 4\] tensor"),
                          (dict(b=b[:3]), ValueError, r"backend_pca_plda: b must be a contiguous float64 \[4, 4\] tensor"),
                          (dict(mu=mu.cpu()), ValueError, r"backend_pca_plda: mu must be a contiguous float64 \[4\] tensor on the rows' device")):
        with pytest.raises(exc, match=what):
            call(**kw)
    assert int(call()["p"][0]) == 2      # and the device still works afterwards
