"""Every branch of the segment-level GEMM kernel (csrc/xv_skinny.hip) at the smallest shapes that reach it, each output against a float64
evaluation of the same operation on the same float32 inputs (tests/segment_ref.py) within a bound derived from the kernel's own order of
operations - per element or per channel, never relative to the tensor's largest entry.  A row first asserts its plan (splits, stages of a
full workgroup, stages of the last split, valid floats of the last stage) through the restatement of tests/test_segment_plans.py and the
library's hook, so a row that drifts to another branch after a plan change fails by name.

The C entry points take ws, ws_bytes and tickets, so the GPU backend (class GpuOps) calls them through _lib.call with buffers of its own: a
workspace filled with NaN before every launch (every slab word a launch reads, it must have written), a ticket buffer checked to be all
zero after every launch, operands and results as NaN-surrounded pitched views whose pads must still be NaN afterwards.  The rows are
functions of a backend; tests/test_segment_ref.py hands them a plain float32 NumPy evaluation first.  $XV_BOUNDS_OUT names a file that
receives the largest ratio to its bound per form and the wall time of the module."""
import ctypes as C
import time

import numpy as np
import pytest

import bn_pool_ref as R
import segment_ref as S
import test_gpu_attention_forms as GA
import test_gpu_bn_pool_forms as G
import test_segment_plans as P
from test_gpu_bn_pool_forms import seed_of, slope_of

pytestmark = pytest.mark.gpu

EPS, MOMENTUM = 1e-3, 0.99
LEDGER = R.Ledger()
SHARES = {}
WS_BYTES = P.SK_TARGET_WGS * P.SLAB_BYTES      # 4 MB: splits x tiles never exceeds 256, so this workspace caps no plan ("large")


def note_share(form, row, amb):
    share = float(np.mean(amb)) if amb.size else 0.0
    SHARES[form] = max(SHARES.get(form, 0.0), share)
    assert share <= R.MAX_AMBIGUOUS_SHARE, "%s: %.3g of the elements are mask-ambiguous (cap %.0e): change the seed" % (row, share, R.MAX_AMBIGUOUS_SHARE)


def write_ledger(tag, seconds):
    G.write_ledger(tag, seconds, LEDGER, SHARES, "segment forms")
    LEDGER.worst.clear()      # (also without $XV_BOUNDS_OUT: the CPU module of these rows shares this ledger)
    SHARES.clear()


def plan_of(m, n, k, ws_bytes=WS_BYTES):
    """The restated plan, held against the library's."""
    assert P.lib_segment_plan(m, n, k, ws_bytes) == P.segment_plan(m, n, k, ws_bytes)
    return P.segment_stages(m, n, k, ws_bytes)


class GpuOps(GA.GpuOps):
    """float32 NumPy in, float32 NumPy out, through the C entry points on buffers of this class."""

    def __init__(self):
        super(GpuOps, self).__init__()
        t = self.torch
        self.ws = t.empty(WS_BYTES // 4, dtype=t.float32, device=self.dev_name)
        self.tickets = t.zeros(1024, dtype=t.int32, device=self.dev_name)

    def guard(self):
        self.ws.fill_(float("nan"))      # stream-ordered: no host wait

    def tickets_clear(self, what):
        assert int(self.tickets.abs().sum().item()) == 0, "%s left a ticket behind" % what

    def pitched(self, a, pitch):
        return None if a is None else self.view(a, pitch)

    def row_term(self, row_term, ldx):
        if row_term is None:
            return (None, None, None), 0
        coef, norm, x = row_term
        dx = self.pitched(x, ldx)
        return (self.vec(coef), self.vec(norm), dx), dx.stride(0)

    def upload_gemm(self, a, bt, bias, row_term, ws_bytes, pitches):
        """Everything a launch reads or writes, on the device (an upload makes the host wait for the stream, so all of them come first).
        -> the argument list of xv_segment_gemm behind the stream, with the tensors kept alive in it; the whole result buffer; m, n, ldc"""
        m, k = a.shape
        n = bt.shape[0]
        pt = pitches or {}
        da, db, dbias = self.pitched(a, pt.get("lda")), self.pitched(bt, pt.get("ldb")), self.vec(bias)
        (rc, rn, rx), ldx = self.row_term(row_term, pt.get("ldx"))
        ldc = pt.get("ldc") or n
        cbuf = self.torch.full(((m + 2) * ldc,), float("nan"), dtype=self.torch.float32, device=self.dev_name)
        args = (da, da.stride(0), db, db.stride(0), m, n, k, dbias, rc, rn, rx, ldx, cbuf, ldc, self.ws,
                C.c_size_t(WS_BYTES if ws_bytes is None else ws_bytes), self.tickets)
        return args, cbuf, m, n, ldc

    def launch_gemm(self, args):
        """The NaN refill of the workspace and the launch, both in stream order: nothing here waits for the device."""
        p = self.ops._p
        self.guard()
        self.lib.call("xv_segment_gemm", self.stream(), *[p(v) if (v is None or self.torch.is_tensor(v)) else v for v in args])

    def collect_gemm(self, cbuf, m, n, ldc):
        full = self.host(cbuf).reshape(m + 2, ldc)
        c = full[:m, :n].copy()
        full[:m, :n] = np.nan
        assert np.all(np.isnan(full)), "xv_segment_gemm wrote outside its m x n view (pitch %d)" % ldc
        return c

    def gemm(self, a, bt, bias=None, row_term=None, ws_bytes=None, pitches=None):
        args, cbuf, m, n, ldc = self.upload_gemm(a, bt, bias, row_term, ws_bytes, pitches)
        self.launch_gemm(args)
        c = self.collect_gemm(cbuf, m, n, ldc)
        self.tickets_clear("xv_segment_gemm")
        return c

    def gemm_queue(self, problems):
        """The launches back to back on one stream: one ticket buffer, one workspace refilled with NaN in stream order.  Every operand and result
        buffer of every problem is on the device before the first launch; between the launches there is nothing but the stream-ordered fill;
        results are read and the tickets checked only after the last."""
        queued = [self.upload_gemm(*p) for p in problems]
        self.torch.cuda.synchronize()
        for q in queued:
            self.launch_gemm(q[0])
        out = [self.collect_gemm(*q[1:]) for q in queued]
        self.tickets_clear("a queue of xv_segment_gemm launches")
        return out

    def bn_forward(self, x, wt, bias, gamma, beta, eps, momentum, unbiased, mm, mv, relu, slope=None, want_a=True, pitches=None):
        m, k = x.shape
        n = wt.shape[0]
        pt = pitches or {}
        p = self.ops._p
        dx, dw = self.pitched(x, pt.get("lda")), self.pitched(wt, pt.get("ldb"))
        vin = [self.vec(v) for v in (bias, gamma, beta, mm, mv)]
        zb, z = self.out(m * n)
        ab, a = self.out(m * n)
        vout = [self.out(n) for _ in range(4)]
        self.guard()
        with self.activation(slope):
            self.lib.call("xv_segment_affine_bn_forward", self.stream(), p(dx), dx.stride(0), p(dw), dw.stride(0), m, n, k, p(vin[0]), p(vin[1]),
                          p(vin[2]), float(eps), float(momentum), int(unbiased), p(vin[3]), p(vin[4]), p(z), p(vout[0][1]), p(vout[1][1]),
                          p(vout[2][1]), p(vout[3][1]), int(relu), p(a if want_a else None), p(self.ws), C.c_size_t(WS_BYTES), p(self.tickets))
        out = dict(z=self.done(zb, m * n, "bn forward (z)").reshape(m, n))
        for key, (buf, _) in zip(("mean", "invstd", "scale", "shift"), vout):
            out[key] = self.done(buf, n, "bn forward (%s)" % key)
        if want_a:
            out["a"] = self.done(ab, m * n, "bn forward (a)").reshape(m, n)
        else:
            assert np.all(np.isnan(self.host(ab))), "xv_segment_affine_bn_forward wrote an activation nobody asked for"
        if mm is not None:
            out["moving_mean"], out["moving_var"] = self.host(vin[3]).copy(), self.host(vin[4]).copy()
        self.tickets_clear("xv_segment_affine_bn_forward")
        return out

    def bn_backward(self, dy, wt, row_term, z, gamma, mean, invstd, scale, shift, relu, slope=None, want_dalpha=False, want_dbias=True, pitches=None):
        m, k = dy.shape
        n = wt.shape[0]
        pt = pitches or {}
        p = self.ops._p
        ddy, dw = self.pitched(dy, pt.get("lda")), self.pitched(wt, pt.get("ldb"))
        (rc, rn, rx), ldx = self.row_term(row_term, pt.get("ldx"))
        dzin = self.view(z)
        vin = [self.vec(v) for v in (gamma, mean, invstd, scale, shift)]
        zb, dz = self.out(m * n)
        vout = [self.out(n) for _ in range(4)]      # dgamma, dbeta, dbias, dalpha
        self.guard()
        with self.activation(slope, vout[3][1] if want_dalpha else None):
            self.lib.call("xv_segment_dgrad_bn_backward", self.stream(), p(ddy), ddy.stride(0), p(dw), dw.stride(0), m, n, k, p(rc), p(rn), p(rx), ldx,
                          p(dzin), p(vin[0]), p(vin[1]), p(vin[2]), p(vin[3]), p(vin[4]), int(relu), p(dz), p(vout[0][1]), p(vout[1][1]),
                          p(vout[2][1] if want_dbias else None), p(self.ws), C.c_size_t(WS_BYTES), p(self.tickets))
        out = dict(dz=self.done(zb, m * n, "bn backward (dz)").reshape(m, n), dgamma=self.done(vout[0][0], n, "bn backward (dgamma)"),
                   dbeta=self.done(vout[1][0], n, "bn backward (dbeta)"))
        for key, want, (buf, _) in (("dbias", want_dbias, vout[2]), ("dalpha", want_dalpha, vout[3])):
            if want:
                out[key] = self.done(buf, n, "bn backward (%s)" % key)
            else:
                assert np.all(np.isnan(self.host(buf))), "xv_segment_dgrad_bn_backward wrote a %s nobody asked for" % key
        self.tickets_clear("xv_segment_dgrad_bn_backward")
        return out


@pytest.fixture(scope="module")
def be():
    t0 = time.time()
    yield GpuOps()
    write_ledger("gpu", time.time() - t0)


PITCHED = dict(lda=4, ldb=8, ldx=3, ldc=5)      # floats added to the row length (lda, ldb stay multiples of 4)


def pitches_of(n, k, on=True):
    return dict(lda=k + PITCHED["lda"], ldb=k + PITCHED["ldb"], ldx=n + PITCHED["ldx"], ldc=n + PITCHED["ldc"]) if on else None


# =========================================================================================== plain epilogue: splits and stages
TWO_SLABS = P.slab_bytes(64, 2)
SPLIT_CASES = [      # n, k, ws_bytes -> splits, stages of a full workgroup, stages of the last split, valid floats of its last stage
    ((32, 4, WS_BYTES), (1, 1, 1, 4)), ((32, 32, WS_BYTES), (1, 1, 1, 32)), ((32, 36, WS_BYTES), (1, 2, 2, 4)), ((32, 60, WS_BYTES), (1, 2, 2, 28)),
    ((32, 64, WS_BYTES), (1, 2, 2, 32)), ((32, 96, WS_BYTES), (1, 3, 3, 32)), ((32, 100, WS_BYTES), (1, 4, 4, 4)),
    ((32, 128, WS_BYTES), (2, 2, 2, 32)), ((32, 192, WS_BYTES), (3, 2, 2, 32)), ((32, 256, WS_BYTES), (4, 2, 2, 32)),
    ((32, 320, WS_BYTES), (5, 2, 2, 32)), ((32, 448, WS_BYTES), (7, 2, 2, 32)), ((32, 512, WS_BYTES), (8, 2, 2, 32)),
    ((32, 576, WS_BYTES), (9, 2, 2, 32)),
    ((32, 128, 0), (1, 4, 4, 32)), ((32, 160, 0), (1, 5, 5, 32)), ((32, 224, 0), (1, 7, 7, 32)),      # rotation remainders 1, 2, 1 behind a full round
    ((64, 452, WS_BYTES), (5, 3, 3, 4)), ((33, 196, WS_BYTES), (3, 3, 1, 4)), ((96, 544, WS_BYTES), (6, 3, 2, 32)),
    ((64, 512, TWO_SLABS), (2, 8, 8, 32)), ((64, 512, TWO_SLABS - 1), (1, 16, 16, 32)), ((64, 512, 0), (1, 16, 16, 32)),
]
SPLIT_PARAMS = [(shape, want, fam) for shape, want in SPLIT_CASES for fam in ("base", "hetero")]


def row_plain_splits(be, shape, want, family):
    """xv_segment_gemm at M = 128 with pitched, NaN-padded operands and result: every count of the slab sum (1 ... 9 splits: by-four rounds with
    remainders 0 ... 3, and a remainder after a round at 5, 6, 7, 9), every tail of the three-stage rotation (1, 2, 3, 4, 5, 7, 8, 16 stages), a
    partial last stage of 4 and of 28 floats alone and behind a short last split, and the workspace cap at, one byte under and far under two
    slabs.  L = k_chunk + splits (S.gemm_bound).  A split launch agrees with the same problem at ws_bytes = 0 within the sum of the two bounds;
    every launch agrees with its own repeat bit for bit."""
    n, k, ws = shape
    m = 128
    s = plan_of(m, n, k, ws)
    assert (s["splits"], s["stages"], s["last_stages"], s["last_valid"]) == want, s
    rs = np.random.RandomState(seed_of("plain splits", n, k, ws, family))
    a, bt, bias = S.make_operands(rs, m, n, k, family)
    pt = pitches_of(n, k)
    got = be.gemm(a, bt, bias, None, ws, pt)
    ref, bound = S.gemm(a, bt, bias), S.gemm_bound(a, bt, bias, None, s["k_chunk"], s["splits"])
    form = "segment gemm, %d split%s" % (s["splits"], "" if s["splits"] == 1 else "s")
    LEDGER.check(form, "c (%d stages, last %d with %d floats)" % want[1:], got, ref,
                 LEDGER.capped(bound, ref, 2e-5) if family == "base" else bound)      # test_segment_gemm_and_fused_batchnorm: 2e-5 of the largest entry
    LEDGER.exact(form, "repeat", be.gemm(a, bt, bias, None, ws, pt), got)
    if s["splits"] > 1:
        one = plan_of(m, n, k, 0)
        assert one["splits"] == 1
        twin = be.gemm(a, bt, bias, None, 0, pt)
        LEDGER.check("segment gemm, split against unsplit", "c", got, twin, bound + S.gemm_bound(a, bt, bias, None, one["k_chunk"], 1))


@pytest.mark.parametrize("shape,want,family", SPLIT_PARAMS)
def test_plain_splits_and_stages(be, shape, want, family):
    row_plain_splits(be, shape, want, family)


# =========================================================================================== plain epilogue: rows and columns
SHAPE_M = (1, 2, 4, 5, 31, 32, 33, 36, 64, 127, 128)
SHAPE_N = (1, 31, 32, 33, 63, 65)
SHAPE_CASES = [(bias, row, fam) for bias in (False, True) for row in (False, True) for fam in ("base", "hetero")]


def row_plain_shapes(be, with_bias, with_row, family):
    """M in {1, 2, 4, 5, 31, 32, 33, 36, 64, 127, 128}: the accumulator-row (4, 8), half-wave and wave (32) boundaries, M <= 32 leaving three waves
    without a valid row; N in {1, 31, 32, 33, 63, 65} around the 32-column tile; K = 196: three splits, the last a single 4-float stage.  Bias
    absent / present, the row term absent / present (norm[0] = 0, a negative coefficient); pitched and contiguous views alternate."""
    k = 196
    rs = np.random.RandomState(seed_of("plain shapes", with_bias, with_row, family))
    for m in SHAPE_M:
        for n in SHAPE_N:
            s = plan_of(m, n, k)
            assert (s["splits"], s["last_stages"], s["last_valid"]) == (3, 1, 4), s
            a, bt, bias = S.make_operands(rs, m, n, k, family)
            bias = bias if with_bias else None
            row = S.make_row_term(rs, m, n, family) if with_row else None
            pt = pitches_of(n, k, (m + n) % 2 == 1)
            got = be.gemm(a, bt, bias, row, None, pt)
            ref, bound = S.gemm(a, bt, bias, row), S.gemm_bound(a, bt, bias, row, s["k_chunk"], s["splits"])
            form = "segment gemm%s%s" % (", bias" if with_bias else "", ", row term" if with_row else "")
            LEDGER.check(form, "c", got, ref, LEDGER.capped(bound, ref, 2e-5) if (family == "base" and m >= 31 and n >= 31) else bound)
            LEDGER.exact(form, "repeat", be.gemm(a, bt, bias, row, None, pt), got)


@pytest.mark.parametrize("with_bias,with_row,family", SHAPE_CASES)
def test_plain_rows_and_columns(be, with_bias, with_row, family):
    row_plain_shapes(be, with_bias, with_row, family)


def row_plain_clamp(be, family):
    """N = 8 193, K = 8, M = 3: 257 column tiles, 256 / 257 = 0 splits clamped to one."""
    m, n, k = 3, 8193, 8
    s = plan_of(m, n, k)
    assert (s["tiles"], s["splits"], s["stages"], s["last_valid"]) == (257, 1, 1, 8)
    rs = np.random.RandomState(seed_of("plain clamp", family))
    a, bt, bias = S.make_operands(rs, m, n, k, family)
    row = S.make_row_term(rs, m, n, family)
    got = be.gemm(a, bt, bias, row, None, pitches_of(n, k))
    LEDGER.check("segment gemm, 257 tiles", "c", got, S.gemm(a, bt, bias, row), S.gemm_bound(a, bt, bias, row, s["k_chunk"], 1))


@pytest.mark.parametrize("family", ["base", "hetero"])
def test_plain_tile_clamp(be, family):
    row_plain_clamp(be, family)


# =========================================================================================== BatchNorm forward epilogue
BN_SHAPES = [(1, 33, 68), (2, 33, 196), (5, 31, 320), (37, 65, 452), (128, 32, 512)]
BN_PLANS = {      # shape -> splits, stages of a full workgroup, stages of the last split, valid floats of its last stage
    (1, 33, 68): (1, 3, 3, 4), (2, 33, 196): (3, 3, 1, 4), (5, 31, 320): (5, 2, 2, 32), (37, 65, 452): (5, 3, 3, 4), (128, 32, 512): (8, 2, 2, 32)}
BN_BWD_PLANS = {4: (1, 1, 1, 4), 64: (1, 2, 2, 32), 196: (3, 3, 1, 4)}      # K of the gradient GEMM -> the same, at every N of BN_SHAPES
BN_FWD_CASES = [(shape, kind, fam) for shape in BN_SHAPES for kind in G.KINDS for fam in ("base", "hetero")]
# One row in the heterogeneous family: y = beta only after z scale cancels against shift, and at a channel scale of 1000 the rounding of that
# cancellation comes near beta - whether a sign is ambiguous is then a matter of the seed (note_share names the row); a row over the cap gets
# another seed here, not an exclusion.
RESEED = {("bn backward", (1, 33, 68), "prelu", "hetero"): (2,)}


def asserted_plan(m, n, k, want):
    s = plan_of(m, n, k)
    assert (s["splits"], s["stages"], s["last_stages"], s["last_valid"]) == want, ((m, n, k), s)
    return s


def row_bn_forward(be, shape, kind, family):
    """xv_segment_affine_bn_forward: (M, N, K) in {(1, 33, 68), (2, 33, 196), (5, 31, 320), (37, 65, 452), (128, 32, 512)}; no activation, ReLU, a
    prelu vector of both signs, the constant 0.2 slope; unbiased 0 / 1; moving statistics given / NULL; bias NULL once; a NULL once (z and the
    vectors still right); a negative gamma.  z against the GEMM; the statistics against S.bn_forward on the z the launch returned
    (L = 16 + 1 + 2); a against the activation of z scale + shift with the launch's own scale and shift, mask-ambiguous elements left out.
    M = 1: the variance is exactly 0, the moving variance keeps the biased value, a = act(beta) within the rounding of the cancellation."""
    m, n, k = shape
    s = asserted_plan(m, n, k, BN_PLANS[shape])
    rs = np.random.RandomState(seed_of("bn forward", shape, kind, family, *RESEED.get(("bn forward", shape, kind, family), ())))
    x, wt, bias = S.make_operands(rs, m, n, k, family)
    gamma, beta = R.make_affine(rs, n, family, negative=1)
    relu, slope, _ = slope_of(rs, kind, n)
    options = [(unbiased, moving, True, True) for unbiased in (0, 1) for moving in (True, False)] + [(1, True, False, True), (0, True, True, False)]
    for unbiased, moving, with_bias, want_a in options:
        mm, mv = (R.f32(rs.randn(n)), R.f32(rs.rand(n) + 0.5)) if moving else (None, None)
        b = bias if with_bias else None
        got = be.bn_forward(x, wt, b, gamma, beta, EPS, MOMENTUM, unbiased, mm, mv, relu, slope, want_a, pitches_of(n, k, unbiased == 1))
        form = "bn forward epilogue, %d split%s" % (s["splits"], "" if s["splits"] == 1 else "s")
        cap = family == "base" and m >= 37      # test_segment_gemm_and_fused_batchnorm: 2e-5 (z), 1e-4 (the rest) of the largest entry
        zref, zb = S.gemm(x, wt, b), S.gemm_bound(x, wt, b, None, s["k_chunk"], s["splits"])
        LEDGER.check(form, "z", got["z"], zref, LEDGER.capped(zb, zref, 2e-5) if cap else zb)
        ref, bound = S.bn_forward_bound(got["z"], gamma, beta, EPS, MOMENTUM, unbiased, mm, mv)
        for key in bound:
            LEDGER.check(form, key + (" (unbiased)" if key == "moving_var" and unbiased else ""), got[key], ref[key],
                         LEDGER.capped(bound[key], ref[key], 1e-4) if cap else bound[key])
        if m == 1:
            if moving:
                LEDGER.check(form, "one row: moving_var keeps the biased value", got["moving_var"], R.f64(mv) * float(np.float32(MOMENTUM)),
                             2 * R.U * np.abs(R.f64(mv)))
        if not want_a:
            continue
        _, _, amb, mag = R.pre_activation(got["z"], got["scale"], got["shift"])
        amb = amb if relu else np.zeros_like(amb)
        aref, ab = R.bn_apply(got["z"], got["scale"], got["shift"], relu, slope), R.bn_apply_bound(got["z"], got["scale"], got["shift"], relu, slope)
        LEDGER.check(form, "a (%s)" % kind, got["a"], aref, LEDGER.capped(ab, aref, 1e-4) if cap else ab, ~amb)
        note_share(form, "bn forward %r %s %s" % (shape, kind, family), amb)
        if m == 1:
            zs = np.abs(R.f64(got["z"]) * R.f64(got["scale"]))
            cancel = (4 * R.U * zs + 2 * R.U * (np.abs(R.f64(beta)) + np.abs(R.f64(got["shift"])))) * R.slope_mag(relu, slope, n)
            want = R.act(R.f64(beta)[None, :], relu, slope)
            LEDGER.check(form, "one row: a = act(beta)", got["a"], want, cancel + R.U * np.abs(want), np.abs(R.f64(beta))[None, :] > cancel)


@pytest.mark.parametrize("shape,kind,family", BN_FWD_CASES)
def test_bn_forward_epilogue(be, shape, kind, family):
    row_bn_forward(be, shape, kind, family)


# =========================================================================================== BatchNorm backward epilogue
BN_BWD_CASES = BN_FWD_CASES


def row_bn_backward(be, shape, kind, family):
    """xv_segment_dgrad_bn_backward on the layer shapes of the forward rows (M x N; the third number is not used), the gradient GEMM over K in
    {4, 64, 196} (one stage of 4 floats; two stages; three splits): no activation, ReLU, prelu (dalpha asserted), lrelu (a slope without a
    dalpha buffer); the row term absent / present; dbias NULL once; column 0 of z constant over the batch (xhat = 0, invstd = 1 / sqrt(eps));
    a negative gamma.  d a is never written: the reference forms it in float64 from the operands, its GEMM bound E is carried through every
    output (S.bn_backward, S.bn_backward_dz); z, mean, invstd, scale and shift are handed in."""
    m, n, _ = shape
    rs = np.random.RandomState(seed_of("bn backward", shape, kind, family, *RESEED.get(("bn backward", shape, kind, family), ())))
    z = R.make_z(rs, m, n, family)
    z[:, 0] = z[0, 0]
    gamma, beta = R.make_affine(rs, n, family, negative=1)
    mean, invstd, scale, shift = S.handed_statistics(z, gamma, beta, EPS)
    mean[0], invstd[0] = z[0, 0], np.float32(1) / np.sqrt(np.float32(EPS), dtype=np.float32)
    scale[0] = gamma[0] * invstd[0]
    shift[0] = np.float32(R.f64(beta[0]) - R.f64(mean[0]) * R.f64(scale[0]))
    relu, slope, want_dalpha = slope_of(rs, kind, n)
    for k in (4, 64, 196):
        for with_row in (False, True):
            s = asserted_plan(m, n, k, BN_BWD_PLANS[k])
            dy, w2, _ = S.make_operands(rs, m, n, k, family)
            w2 = R.f32(w2 * np.sqrt(k) / 8)      # (randn / 8: the scaling of the earlier row)
            row = S.make_row_term(rs, m, n, family) if with_row else None
            want_dbias = not (k == 4 and not with_row)
            got = be.bn_backward(dy, w2, row, z, gamma, mean, invstd, scale, shift, relu, slope, want_dalpha, want_dbias, pitches_of(n, k, with_row))
            da, E = S.gemm(dy, w2, None, row), S.gemm_bound(dy, w2, None, row, s["k_chunk"], s["splits"])
            red = S.bn_backward(da, E, z, gamma, mean, invstd, scale, shift, relu, slope)
            assert np.all(red["xhat"][:, 0] == 0)
            form = "bn backward epilogue %s%s" % (kind, ", row term" if with_row else "")
            cap = family == "base" and m >= 37 and not red["ambiguous"].any()      # test_segment_gemm_and_fused_batchnorm: 1e-4 / 2e-4 of the largest entry
            for key in ("dbeta", "dgamma") + (("dalpha",) if want_dalpha else ()):
                b = red["b_" + key]
                LEDGER.check(form, key, got[key], red[key], LEDGER.capped(b, red[key], 1e-4) if cap else b)
            dz_ref, b_dz = S.bn_backward_dz(red, z, gamma, mean, invstd, got["dbeta"], got["dgamma"])
            LEDGER.check(form, "dz", got["dz"], dz_ref, LEDGER.capped(b_dz, dz_ref, 2e-4) if cap else b_dz, ~red["ambiguous"])
            if want_dbias:
                LEDGER.check(form, "dbias", got["dbias"], np.zeros(n), S.dbias_bound(red, gamma, invstd))
            note_share(form, "bn backward %r %s %s k %d" % (shape, kind, family, k), red["ambiguous"])


@pytest.mark.parametrize("shape,kind,family", BN_BWD_CASES)
def test_bn_backward_epilogue(be, shape, kind, family):
    row_bn_backward(be, shape, kind, family)


# =========================================================================================== ticket hygiene
QUEUE = [(32, 576, 9), (33, 36, 1), (64, 452, 5), (96, 128, 2)]      # n, k -> splits


def row_ticket_hygiene(be, family):
    """Four launches of 9, 1, 5 and 2 splits and different N queued back to back on one stream: one ticket buffer, one workspace refilled with
    NaN in stream order, no host wait between them (the backend uploads every problem first).  Each result is bit-identical to the same launch run alone, and the tickets end at zero."""
    rs = np.random.RandomState(seed_of("queue", family))
    problems = []
    for n, k, splits in QUEUE:
        assert plan_of(128, n, k)["splits"] == splits
        a, bt, bias = S.make_operands(rs, 128, n, k, family)
        problems.append((a, bt, bias, None, None, pitches_of(n, k)))
    alone = [be.gemm(*p) for p in problems]
    for rep in range(3):
        for got, want, (n, k, splits) in zip(be.gemm_queue(problems), alone, QUEUE):
            LEDGER.exact("segment gemm, queued launches", "%d splits" % splits, got, want)


@pytest.mark.parametrize("family", ["base", "hetero"])
def test_ticket_hygiene(be, family):
    row_ticket_hygiene(be, family)
