"""The loss head against the float64 oracle, one row per launch form x loss kind, with rows planted on every per-row branch
(csrc/xv_loss.hip margin_softmax_rows_kernel, col_inv_norm_kernel, loss_weight_bwd_kernel, the MHE kernels).

The row kernel is fed fp32 logits directly and oracle.margin_softmax_rows_ref runs on the same logits upcast to float64, so no GEMM
rounding sits between them.  Each row first asserts its form through xv_debug_softmax_rows_form and the restatement of
tests/test_loss_plans.py - a row that has drifted off its form FAILS and says so.  Then, per row r: the row loss within
1e-6 + 2e-6 |ref|, dlogits within 5e-6 Frobenius / 2e-5 max of the tensor scale, d||x|| within 2e-5 of the row's scale
fa (|phi| + |dphi cos|) / rows, and the mean loss.  fp32 carries a logit u to 6e-8 |u|, and the softmax turns that absolute error into
a relative one on every probability, so each of these bounds grows by 4e-7 M_r (M_r: the row's largest |updated logit|; 2e-6 at the
|x| = 5 of the planted rows, 4e-4 on the |x| = 1e3 row) and the Frobenius bound leaves out rows with M_r > 64.  The pad columns
[N, ldl) of the logits hold NaN, which must not reach any output; the pad columns of dlogits, poisoned before the launch, must come back
exactly 0.  A second launch must reproduce the first bit for bit.

Coverage (form x kind; every kind on every form, rows = 1, 37, 128, lambda 0 / 0.5 / 1e3 rotating over the rows counts):
  RQ = 8   row in registers, 8 float4 per thread     ldl = 8192 (the last pitch), N = 8189
  RQ = 16  row in registers, 16 float4 per thread    ldl = 8196 (the first pitch), N = 8193; ldl = 16384 (the last), N = 16381
  RQ = 0   three passes                              ldl = 16388 (the first past RQ = 16), N = 16385; ldl = N = 1001 (odd);
                                                     ldl = 1004, N = 1001, logits 4 bytes off 16-byte alignment
  kinds: softmax with bias, A-Softmax m = 1 (no margin) / 2 / 4, AM m = 0 / 0.35, ArcFace m = 0 / 0.5
Planted rows: cos = +1 and -1 exactly (|x| = 5 exactly in fp32), |cos_raw| = 1.25 / 1.5 (the clamp, cm = 0), cos = -0.9 / -0.3 / 0.3
/ 0.9 (the four sign regions of A-Softmax m = 4), ArcFace cos(pi - m) +- 0.01, x = 0 (d||x|| exactly 0), |x| = 1e3 (logits to +-1e3);
labels at column 0, N - 1, 7 (the last lane of a float4), 1023 and 2047 (the last lanes of a 1 024-column register stride).

Weight normalisation (xv_loss_prep_weight -> xv_affine_wgrad -> xv_loss_weight_backward, and xv_mhe_loss / xv_mhe_add_grad) at C = 36,
N = 1001 with columns of norm 0, 5e-7 (clamped), 1e-6 with the smallest fp32 ss >= 1e-12f, 1.005e-6, 1.02e-6, 1e-3 and O(1), compared
column by column against oracle.l2_normalize_w_backward / mhe_loss with TF's fp32 liveness (ss >= 1e-12f).

Engine rows in the 8 193 ... 16 385 speaker range (tests/test_gpu_engine.py::_check_train_step), each asserting the form of its
pitch align(N, 4): RQ = 16 for softmax N = 8193, A-Softmax m = 4 N = 12289, AM + feature_norm N = 16381; RQ = 0 for ArcFace N = 16385.
"""
import numpy as np
import pytest
import torch

from oracle import xvector_oracle as O
from tests.test_gpu_ops import assert_close, dev, host
from tests.test_loss_plans import FORM_NAMES, RQ8, RQ16, THREE_PASS, align4, lib_form, rows_form

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
C_FEAT = 24
E32 = float(np.float32(1e-12))       # loss.py's epsilons are float32 constants

KIND_IDS = {"softmax": 0, "asoftmax": 1, "additive_margin_softmax": 2, "additive_angular_margin_softmax": 3}
ARC = "additive_angular_margin_softmax"
KINDS = [("softmax", 0), ("asoftmax", 1), ("asoftmax", 2), ("asoftmax", 4), ("additive_margin_softmax", 0.0),
         ("additive_margin_softmax", 0.35), (ARC, 0.0), (ARC, 0.5)]
# (name, ldl, N, logits offset in floats, form)
FORMS = [("rq8-ldl8192", 8192, 8189, 0, RQ8),
         ("rq16-ldl8196", 8196, 8193, 0, RQ16),
         ("rq16-ldl16384", 16384, 16381, 0, RQ16),
         ("rq0-ldl16388", 16388, 16385, 0, THREE_PASS),
         ("rq0-ldl1001-odd", 1001, 1001, 0, THREE_PASS),
         ("rq0-logits-off4", 1004, 1001, 1, THREE_PASS)]
ROWS = (1, 37, 128)
LAMS = (0.0, 0.5, 1e3)


@pytest.fixture(scope="module")
def ops():
    from tf_kaldi_speaker_amd import ops as m
    return m


def plants(kind, m, n):
    """(label, cosine, |x|) of the planted rows; label None: random, |x| = 5: x = (3, 4, 0, ...), exact in fp32"""
    out = [(n - 1, 1.0, 5.0), (0, -1.0, 5.0), (7, 1.25, 5.0), (1023 % n, -1.5, 5.0), (2047 % n, -0.9, 5.0), (None, -0.3, 5.0),
           (None, 0.3, 5.0), (None, 0.9, 5.0)]
    if kind == ARC and m > 0:
        edge = float(np.cos(np.pi - m))
        out += [(None, edge + 0.01, 5.0), (None, edge - 0.01, 5.0)]
    out += [(None, 0.0, 0.0), (None, None, 1e3)]
    return out


def make_case(kind, m, n, rows, seed):
    """fp32 x [rows, C_FEAT], logits [rows, n], int32 labels.  Logits are cos * |x| as x . wn would give (plus a bias for softmax)."""
    rs = np.random.RandomState(seed)
    labels = rs.randint(0, n, rows)
    norms = rs.uniform(2.0, 12.0, rows)
    cos = rs.uniform(-1.0, 1.0, (rows, n))
    tgt = rs.uniform(-0.95, 0.95, rows)
    x = rs.randn(rows, C_FEAT)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    pl = plants(kind, m, n)
    if rows == 1:
        pl = pl[seed % len(pl):][:1]
    for r, (y, c, nrm) in enumerate(pl[:rows]):
        if y is not None:
            labels[r] = y
        if c is not None:
            tgt[r] = c
        norms[r] = nrm
        x[r] = 0.0
        x[r, 0], x[r, 1] = 0.6, 0.8
    x = (x * norms[:, None]).astype(np.float32)
    logits = cos * norms[:, None]
    logits[np.arange(rows), labels] = tgt * norms
    if kind == "softmax":
        logits = logits + rs.randn(n)
    return x, logits.astype(np.float32), labels.astype(np.int32)


def row_scales(kind, m, lam, logits, xnorm, labels):
    """M_r = the row's largest |updated logit|, and the d||x|| scale fa (|phi| + |dphi cm craw|) / rows"""
    rows = logits.shape[0]
    big = np.abs(logits).max(axis=1)
    if kind == "softmax" or (kind == "asoftmax" and m == 1):
        return np.maximum(big, 1.0), np.zeros(rows)
    fn = np.maximum(xnorm, 1e-12)
    craw = logits[np.arange(rows), labels] / fn
    cm = (np.abs(craw) <= 1.0).astype(np.float64)
    phi, dphi = O._phi(kind, m, np.clip(craw, -1.0, 1.0))
    fa = 1.0 / (1.0 + lam)
    return np.maximum(np.maximum(big, np.abs(phi) * fn), 1.0), fa * (np.abs(phi) + np.abs(dphi * cm * craw)) / rows


def launch(ops, kind, m, lam, logits_t, n, x_t, labels_t, form):
    rows, ldl = logits_t.shape
    nan = float("nan")
    dlogits = torch.full((rows, ldl), nan, dtype=torch.float32, device=DEV)
    dnorm, row_loss, loss = (torch.full((k,), nan, dtype=torch.float32, device=DEV) for k in (rows, rows, 1))
    got = lib_form(ldl, logits_t.data_ptr(), dlogits.data_ptr())
    assert got == form and rows_form(ldl, logits_t.data_ptr(), dlogits.data_ptr()) == form, \
        "ldl=%d: the library runs %s, the row is meant for %s - move it to a pitch or offset that still reaches %s" % (
            ldl, FORM_NAMES.get(got, got), FORM_NAMES[form], FORM_NAMES[form])
    ops._lib.call("xv_margin_softmax_rows", ops._s(), KIND_IDS[kind], ops._p(logits_t), rows, n, ldl, ops._p(x_t), C_FEAT,
                  ops._p(labels_t), float(m), float(lam), ops._p(dlogits), ops._p(dnorm), ops._p(row_loss), ops._p(loss))
    torch.cuda.synchronize()
    return dlogits, dnorm, row_loss, loss


@pytest.mark.parametrize("kind,m", KINDS, ids=["%s-m%g" % (k.replace("additive_", ""), m) for k, m in KINDS])
@pytest.mark.parametrize("fname,ldl,n,off,form", FORMS, ids=[f[0] for f in FORMS])
def test_row_kernel_form_and_kind(ops, fname, ldl, n, off, form, kind, m):
    fi = [f[0] for f in FORMS].index(fname)
    worst = dict(loss=0.0, dlogits=0.0, dnorm=0.0)
    for ri, rows in enumerate(ROWS):
        lam = LAMS[(ri + fi) % len(LAMS)]
        x, logits, labels = make_case(kind, m, n, rows, seed=1000 * fi + 10 * ri + KINDS.index((kind, m)))
        buf = torch.full((rows * ldl + 4,), float("nan"), dtype=torch.float32, device=DEV)
        lg = buf[off:off + rows * ldl].view(rows, ldl)
        lg[:, :n] = dev(logits)
        x_t, y_t = dev(x), dev(labels, np.int32)
        dl, dn, rl, loss = launch(ops, kind, m, lam, lg, n, x_t, y_t, form)
        again = launch(ops, kind, m, lam, lg, n, x_t, y_t, form)
        for a, b, what in zip((dl, dn, rl, loss), again, ("dlogits", "dnorm", "row_loss", "loss")):
            assert torch.equal(a, b), "%s: a second launch changed %s" % (fname, what)
        dl, dn, rl, loss = host(dl), host(dn), host(rl), host(loss)[0]
        tag = "%s %s m=%g rows=%d lambda=%g" % (fname, kind, m, rows, lam)
        assert np.all(dl[:, n:] == 0), tag + ": pad columns of dlogits not zeroed"
        for t, what in ((dl, "dlogits"), (dn, "dnorm"), (rl, "row_loss")):
            assert np.all(np.isfinite(t)), "%s: %s not finite (a NaN pad column reached it?)" % (tag, what)

        lg64, x64 = logits.astype(np.float64), x.astype(np.float64)
        xnorm = np.sqrt((x64 * x64).sum(axis=1))
        rl_ref, dl_ref, dn_ref = O.margin_softmax_rows_ref(kind, lg64, xnorm, labels, m, lam, clip=(-1.0, 1.0))
        M, dscale = row_scales(kind, m, lam, lg64, xnorm, labels)

        tol = 1e-6 + 2e-6 * np.abs(rl_ref) + 4e-7 * M
        err = np.abs(rl - rl_ref)
        bad = np.nonzero(err > tol)[0]
        assert bad.size == 0, "%s: row_loss rows %s: got %s ref %s" % (tag, bad[:8], rl[bad[:4]], rl_ref[bad[:4]])
        worst["loss"] = max(worst["loss"], (err / tol).max())
        mref = rl_ref.mean()
        assert abs(loss - mref) <= 1e-6 + 2e-6 * abs(mref) + 4e-7 * M.max(), (tag, loss, mref)

        scale = np.abs(dl_ref[:, :n]).max()
        rerr = np.abs(dl[:, :n] - dl_ref[:, :n]).max(axis=1) / (scale * (2e-5 + 4e-7 * M))
        bad = np.nonzero(rerr > 1)[0]
        assert bad.size == 0, "%s: dlogits rows %s off by %s of their bound" % (tag, bad[:8], rerr[bad[:8]])
        ordinary = M <= 64
        if ordinary.any():
            fro = np.linalg.norm(dl[ordinary, :n] - dl_ref[ordinary, :n]) / np.linalg.norm(dl_ref[ordinary, :n])
            assert fro <= 5e-6, "%s: dlogits rel_fro %.3e" % (tag, fro)
        worst["dlogits"] = max(worst["dlogits"], rerr.max())

        if dscale.max() == 0:
            assert np.all(dn == 0), tag + ": d||x|| must be 0 without a margin"
        else:
            assert np.all(dn[xnorm == 0] == 0), tag + ": d||x|| must be 0 where ||x|| < eps"
            derr = np.abs(dn - dn_ref) / np.maximum(dscale * (2e-5 + 4e-7 * M), 1e-30)
            bad = np.nonzero(derr > 1)[0]
            assert bad.size == 0, "%s: dnorm rows %s: got %s ref %s" % (tag, bad[:8], dn[bad[:4]], dn_ref[bad[:4]])
            worst["dnorm"] = max(worst["dnorm"], derr.max())
    print("loss-head %s form=%s %s m=%g: worst error / bound: loss %.3f dlogits %.3f dnorm %.3f" % (
        fname, FORM_NAMES[form], kind, m, worst["loss"], worst["dlogits"], worst["dnorm"]))


def smallest_live_entry():
    """The smallest fp32 v with fl32(v * v) >= 1e-12f: a one-entry column whose fp32 ss is the first live value"""
    e = np.float32(1e-12)
    v = np.float32(1e-6)
    while v * v >= e:
        v = np.nextafter(v, np.float32(0))
    while v * v < e:
        v = np.nextafter(v, np.float32(1))
    return v


# planted columns: (column, norm); "edge" = one entry of smallest_live_entry()
PLANTED = [(3, 0.0), (10, 5e-7), (999, "edge"), (100, 1.005e-6), (500, 1.02e-6), (700, 1e-3), (1000, 1.0)]


def test_weight_normalisation_planted_columns(ops):
    """l2_normalize backward (the A-Softmax / AM / ArcFace weight gradient) and the MHE gradient through it, column by column: a column
    is live exactly when its fp32 ss >= 1e-12f (TF's maximum() and its gradient in float32)."""
    rs = np.random.RandomState(5)
    c, n, rows, l2 = 36, 1001, 32, 1e-2
    w = rs.randn(c, n) * 0.05
    for col, nrm in PLANTED:
        if nrm == "edge":
            w[:, col] = 0.0
            w[17, col] = smallest_live_entry()
        else:
            d = rs.randn(c)
            w[:, col] = d / np.linalg.norm(d) * nrm
    w = w.astype(np.float32)
    ss32 = (w * w).sum(axis=0, dtype=np.float32)
    e = np.float32(1e-12)
    edge = [col for col, nrm in PLANTED if nrm == "edge"][0]
    assert ss32[edge] >= e and np.nextafter(np.float32(w[17, edge]), np.float32(0)) ** 2 < e
    assert ss32[10] < e and ss32[3] == 0 and ss32[100] >= e and ss32[500] >= e
    ss_ref = ss32.astype(np.float64)
    w64 = w.astype(np.float64)

    inv, wn, wnt = ops.loss_prep_weight(dev(w), True)
    ldn = wn.shape[1]
    wn_h, wnt_h, inv_h = host(wn), host(wnt), host(inv)
    assert np.all(wn_h[:, n:] == 0), "pad columns of wn"
    assert np.array_equal(wnt_h, wn_h[:, :n].T), "wnt is not the exact transpose of wn"
    inv_ref = 1.0 / np.sqrt(np.maximum(ss_ref, E32))
    wn_ref = w64 * inv_ref
    for col in range(n):
        assert np.abs(wn_h[:, col] - wn_ref[:, col]).max() <= 2e-6 * max(np.abs(wn_ref[:, col]).max(), 1e-30), ("wn", col)

    x = rs.randn(rows, c).astype(np.float32)
    dl = np.zeros((rows, ldn), np.float32)
    dl[:, :n] = rs.randn(rows, n) * 1e-2
    dwn = ops.affine_wgrad(dev(x).view(rows, 1, c), 1, c, dev(dl), 1, 0, ldn, None, 0.0)[0]       # [c, ldn]
    assert_close(host(dwn)[:, :n], x.astype(np.float64).T @ dl[:, :n].astype(np.float64), name="d wn = x^T dlogits")
    labels = rs.randint(0, n, rows).astype(np.int32)
    labels[:len(PLANTED)] = [col for col, _ in PLANTED]
    lam_mhe = 0.05
    coef = torch.zeros(1 + 2 * c, dtype=torch.float32, device=DEV)
    counts = torch.zeros(n, dtype=torch.int32, device=DEV)
    mhe_out = torch.zeros(1, dtype=torch.float32, device=DEV)
    ops._lib.call("xv_mhe_loss", ops._s(), ops._p(wn), c, n, ldn, ops._p(dev(labels, np.int32)), rows, lam_mhe, ops._p(mhe_out),
                  ops._p(coef), ops._p(counts))
    dwn_mhe = dwn.clone()
    ops._lib.call("xv_mhe_add_grad", ops._s(), ops._p(dwn_mhe), c, n, ldn, ops._p(coef), ops._p(counts))
    mhe_ref, dk_mhe = O.mhe_loss(w64, labels, lam_mhe, eps=E32, ss=ss_ref)
    assert abs(float(host(mhe_out)[0]) - mhe_ref) <= 5e-5 * abs(mhe_ref), ("mhe loss", float(host(mhe_out)[0]), mhe_ref)

    failures = []
    for what, dw_in, extra in (("softmax-loss dW", dwn, 0.0), ("softmax-loss + MHE dW", dwn_mhe, dk_mhe)):
        dw = host(ops.loss_weight_backward(dw_in, wn, inv, dev(w), True, l2))
        ref = O.l2_normalize_w_backward(w64, host(dwn)[:, :n], eps=E32, ss=ss_ref) + extra + l2 * w64
        err = np.abs(dw - ref).max(axis=0) / np.maximum(np.abs(ref).max(axis=0), 1e-30)
        for col, nrm in PLANTED:
            print("weight-norm %s column %d (norm %s, ss %.6e): error / column scale %.3e" % (what, col, nrm, ss32[col], err[col]))
        failures += ["%s column %d (norm %s): %.3e" % (what, col, nrm, err[col]) for col, nrm in PLANTED if err[col] > 2e-5]
        other = np.ones(n, bool)
        other[[col for col, _ in PLANTED]] = False
        assert err[other].max() <= 2e-5, (what, int(np.argmax(np.where(other, err, 0))), err[other].max())
    assert not failures, "planted columns off the oracle (error relative to the column's scale): " + "; ".join(failures)

    # the liveness encoding (include/xvector_hip.h, xv_loss_prep_weight): clamped columns exactly 1e6f, live ones below it
    live = ss32 >= e
    assert np.all(inv_h[~live] == 1e6), inv_h[~live]
    assert np.all(inv_h[live] < 1e6) and np.all(np.abs(inv_h[live] - inv_ref[live]) <= 1e-6 * inv_ref[live])


# (N, oracle / engine config): the engine's pitch align(N, 4) and the form it runs
ENGINE_ROWS = [(8193, RQ16, dict(loss_func="softmax")),
               (12289, RQ16, dict(loss_func="asoftmax", margin_m=4, lambda_min=10, lambda_gamma=1e-5, last_layer_linear=True)),
               (16381, RQ16, dict(loss_func="additive_margin_softmax", margin_m=0.2, feature_norm=True, feature_scaling_factor=30.0,
                                  last_layer_linear=True)),
               (16385, THREE_PASS, dict(loss_func="additive_angular_margin_softmax", margin_m=0.25, lambda_gamma=1e-2, last_layer_linear=True))]


@pytest.mark.parametrize("n,form,kw", ENGINE_ROWS, ids=["N%d-%s" % (r[0], r[2]["loss_func"]) for r in ENGINE_ROWS])
def test_engine_step_in_the_wide_speaker_range(n, form, kw):
    """A training step against the oracle at speaker counts the flagship shapes never reach.  The engine carves its logits and
    dlogits 256-byte aligned, so the form follows from the pitch alone."""
    from tests.test_gpu_engine import _check_train_step
    ldl = align4(n)
    assert lib_form(ldl, 0, 0) == form == rows_form(ldl), "N=%d: the engine runs %s, the row is meant for %s" % (
        n, FORM_NAMES.get(lib_form(ldl, 0, 0)), FORM_NAMES[form])
    _check_train_step(kw, 5, 25, N=n, P=600, D=30, L=128)
