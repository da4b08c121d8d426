"""Every kernel form of BatchNorm (csrc/xv_bn.hip, xv_bn_bwd.hip), statistics pooling and l2_scaling (csrc/xv_pool.hip) at the smallest
shapes at which it can still go wrong, each output against a float64 evaluation of the same operation on the same float32 inputs
(tests/bn_pool_ref.py) within a bound derived from the kernel's own order of operations - per element or per channel, never relative to
the tensor's largest entry.  A row first asserts the form it runs through the restatement of tests/test_bn_plans.py and the library's
own hooks, so a row that silently moves to another kernel fails.

The rows are functions of a backend: the tests here hand them the GPU (class GpuOps), tests/test_bn_pool_ref.py hands the same rows a
plain float32 NumPy evaluation first, which must stay within the same bounds, and checks the share of mask-ambiguous elements.
$XV_BOUNDS_OUT names a file that receives the largest ratio to its bound per form and the wall time of the module."""
import os
import time
import zlib

import numpy as np
import pytest

import bn_pool_ref as R
import test_bn_plans as P

pytestmark = pytest.mark.gpu

EPS = 1e-3
LRELU = 0.2
KINDS = ("none", "relu", "prelu", "lrelu")
LEDGER = R.Ledger()
SHARES = {}                    # form -> largest share of ambiguous elements over its rows


def seed_of(*key):
    return zlib.crc32(repr(key).encode()) & 0x7fffffff


def slope_of(rs, kind, n):
    """-> (relu flag, slope vector or None, d alpha wanted): none | relu | prelu (alpha per channel, both signs) | lrelu (constant 0.2)."""
    if kind == "prelu":
        a = 0.01 + 0.3 * rs.rand(n)
        a[::3] = -a[::3]
        return 1, R.f32(a), True
    if kind == "lrelu":
        return 1, np.full(n, LRELU, np.float32), False
    return int(kind == "relu"), None, False


def note_share(form, row, amb):
    share = float(np.mean(amb)) if amb.size else 0.0
    SHARES[form] = max(SHARES.get(form, 0.0), share)
    assert share <= R.MAX_AMBIGUOUS_SHARE, "%s: %.3g of the elements are mask-ambiguous (cap %.0e): change the seed" % (row, share, R.MAX_AMBIGUOUS_SHARE)


class GpuOps(object):
    """The rows' interface over tf_kaldi_speaker_amd.ops: float32 NumPy in, float32 NumPy out."""
    name = "gpu"

    def __init__(self):
        import torch
        from tf_kaldi_speaker_amd import ops
        self.torch, self.ops, self.dev_name = torch, ops, "cuda:0"

    def dev(self, a):
        return None if a is None else self.torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(self.dev_name)

    def host(self, t):
        self.torch.cuda.synchronize()
        return t.detach().cpu().numpy()

    def view(self, a, pitch=None, offset=0):
        """a [rows][n] as a device view with a row pitch and a base offset in floats; everything around it is NaN."""
        rows, n = a.shape
        pitch = n if pitch is None else pitch
        buf = self.torch.full((offset + rows * pitch + 4,), float("nan"), dtype=self.torch.float32, device=self.dev_name)
        v = buf[offset:offset + rows * pitch].view(rows, pitch)[:, :n]
        v.copy_(self.dev(a))
        return v

    def activation(self, slope, dalpha=None):
        import contextlib
        return self.ops.activation(self.dev(slope), dalpha) if slope is not None else contextlib.nullcontext()

    def col_stats(self, z, layout=None, want_form=None):
        pitch, offset = layout or (None, 0)
        v = self.view(z, pitch, offset)
        part = self.ops.col_stats(v)
        if want_form is not None:
            got = P.lib_col_stats_form(z.shape[1], v.stride(0), v.data_ptr(), part.data_ptr())
            assert got == want_form == P.col_stats_form(z.shape[1], v.stride(0), v.data_ptr(), part.data_ptr()), (got, want_form)
        return self.host(part)

    def bn_finalize(self, part, rows, gamma, beta, eps, momentum, unbiased, mm, mv, with_range=False, relu=True, slope=None):
        d_mm, d_mv = self.dev(mm), self.dev(mv)
        with self.activation(slope):
            res = self.ops.bn_finalize(self.dev(part), rows, self.dev(gamma), self.dev(beta), eps, momentum, unbiased, d_mm, d_mv,
                                       with_range=with_range, relu=relu)
        out = dict(zip(("mean", "invstd", "scale", "shift", "zmin", "zmax", "amax"), (self.host(t) for t in res)))
        if with_range:
            out["amax"] = out["amax"][0]
        if mm is not None:
            out["moving_mean"], out["moving_var"] = self.host(d_mm), self.host(d_mv)
        return out

    def bn_output_range(self, part, rows, scale, shift, relu, slope=None):
        with self.activation(slope):
            zmin, zmax, amax = self.ops.bn_output_range(self.dev(part), rows, self.dev(scale), self.dev(shift), relu)
        return self.host(zmin), self.host(zmax), self.host(amax)[0]

    def bn_inference_scale(self, gamma, beta, mm, mv, eps):
        return tuple(self.host(t) for t in self.ops.bn_inference_scale(self.dev(gamma), self.dev(beta), self.dev(mm), self.dev(mv), eps))

    def bn_apply(self, z, scale, shift, relu, slope=None, ldz=None, lda=None):
        rows, n = z.shape
        v = self.view(z, ldz)
        out = None
        if lda is not None:
            out = self.torch.full((rows, lda), -777.0, dtype=self.torch.float32, device=self.dev_name)
        with self.activation(slope):
            a = self.ops.bn_apply(v, self.dev(scale), self.dev(shift), relu, lda=lda, out=out)
        if lda is not None:
            assert np.all(self.host(out)[:, n:] == -777.0), "bn_apply wrote beyond n columns of a pitched result"
        return self.host(a)

    def bn_backward(self, z, gamma, mean, invstd, scale, shift, relu, slope=None, want_dalpha=False, da=None, segs=None, t=None, pad=0,
                    pooled=None, wpos=None):
        n = z.shape[1]
        d_alpha = self.torch.zeros(n, dtype=self.torch.float32, device=self.dev_name) if want_dalpha else None
        vec = [self.dev(v) for v in (gamma, mean, invstd, scale, shift)]
        with self.activation(slope, d_alpha):
            if pooled is None:
                res = self.ops.bn_relu_backward(self.dev(da), self.dev(z), segs, t, *vec, relu, pad, with_dbias=True)
            else:
                pool_out, dpool, pt, w = pooled
                b = z.shape[0] // pt
                w = None if w is None else self.dev(np.reshape(w, -1))
                if wpos is None:
                    res = self.ops.bn_relu_backward_pooled(self.dev(pool_out), self.dev(dpool), b, pt, self.dev(z), *vec, relu=relu, weights=w)
                else:
                    res = self.ops.bn_relu_backward_pooled_aux(self.dev(pool_out), self.dev(dpool), self.dev(wpos), b, pt, self.dev(z), *vec,
                                                               relu=relu, weights=w)
        out = dict(zip(("dz", "dgamma", "dbeta", "dbias"), (self.host(x) for x in res)))
        if want_dalpha:
            out["dalpha"] = self.host(d_alpha)
        return out

    def stat_pool_forward(self, x):
        return self.host(self.ops.stat_pool_forward(self.dev(x)))

    def stat_pool_forward_bn(self, z, b, t, scale, shift, relu, slope=None, weights=None, aux=True):
        w = None if weights is None else self.dev(np.reshape(weights, -1))
        with self.activation(slope):
            if aux:
                return tuple(self.host(x) for x in self.ops.stat_pool_forward_bn_aux(self.dev(z), b, t, self.dev(scale), self.dev(shift), relu, w))
            return self.host(self.ops.stat_pool_forward_bn(self.dev(z), b, t, self.dev(scale), self.dev(shift), relu, w))

    def stat_pool_backward(self, x, out, dout):
        return self.host(self.ops.stat_pool_backward(self.dev(x), self.dev(out), self.dev(dout)))

    def l2_scaling_forward(self, x, factor):
        return self.host(self.ops.l2_scaling_forward(self.dev(x), factor))

    def l2_scaling_backward(self, x, dy, factor):
        return self.host(self.ops.l2_scaling_backward(self.dev(x), self.dev(dy), factor))


@pytest.fixture(scope="module")
def be():
    t0 = time.time()
    yield GpuOps()
    write_ledger("gpu", time.time() - t0)


def write_ledger(tag, seconds, ledger=None, shares=None, title=None):
    """Appends to $XV_BOUNDS_OUT; the later form modules hand in their own ledger, shares and a title, which are emptied once written: the CPU
    modules record into the ledger of the GPU module whose rows they run, and a section holds the figures of its own run only."""
    path = os.environ.get("XV_BOUNDS_OUT")
    if not path:
        return
    ledger, shares = LEDGER if ledger is None else ledger, SHARES if shares is None else shares
    tag = tag if title is None else "%s, %s" % (title, tag)
    with open(path, "a") as f:
        f.write("# %s: largest |got - ref| / bound per form and output; wall time of the rows %.1f s\n" % (tag, seconds))
        f.write("\n".join(ledger.lines()) + "\n")
        f.write("# %s: largest share of mask-ambiguous elements of a row, per form (cap %.0e)\n" % (tag, R.MAX_AMBIGUOUS_SHARE))
        f.write("\n".join("%-64s %.3g" % kv for kv in sorted(shares.items())) + "\n")
    if title is not None:
        ledger.worst.clear()
        shares.clear()


def statistics(be, z, gamma, beta):
    """mean, invstd, scale, shift of z as the backend's own col_stats + bn_finalize produce them (their rows check them)."""
    part = be.col_stats(z)
    s = be.bn_finalize(part, z.shape[0], gamma, beta, EPS, 0.99, False, None, None)
    return s["mean"], s["invstd"], s["scale"], s["shift"]


# =========================================================================================== forward statistics
COL_STATS_CASES = [(rows, fam) for rows in (1, 7, 128, 129, 300) for fam in ("base", "hetero", "offset")]


def row_col_stats(be, rows, family):
    """col_stats_kernel (n in {1, 30, 33}, an odd pitch, an n % 4 == 0 view offset by one float) and col_stats4_kernel (n in {4, 124, 132}, a
    pitch of n + 4): all four planes per tile.  L = 16 + 8: a thread adds its 16 rows of the 128-row tile in row order, the 8 row lanes are
    then added in lane order - the same in both forms; min and max are exact.  The squares are centred on the float32 tile mean: + count dm^2
    (R.col_stats_bound).  Both forms on the same data agree within the sum of their bounds."""
    rs = np.random.RandomState(seed_of("col_stats", rows, family))
    for n, layout, form in ((4, None, P.FLOAT4), (124, None, P.FLOAT4), (132, None, P.FLOAT4), (132, (136, 0), P.FLOAT4), (4, (8, 0), P.FLOAT4),
                            (1, None, P.SCALAR), (30, None, P.SCALAR), (33, None, P.SCALAR), (30, (35, 0), P.SCALAR), (33, (36, 0), P.SCALAR),
                            (132, (132, 1), P.SCALAR), (124, (127, 0), P.SCALAR)):
        z = R.make_z(rs, rows, n, family)
        got = be.col_stats(z, layout, form)
        ref, (bound, _) = R.col_stats(z), R.col_stats_bound(z)
        name = "col_stats %s" % ("float4" if form == P.FLOAT4 else "scalar")
        LEDGER.check(name, "sum", got[0], ref[0], bound[0])
        LEDGER.check(name, "centred squares", got[1], ref[1], bound[1])
        LEDGER.exact(name, "min", got[2], R.f32(ref[2]))
        LEDGER.exact(name, "max", got[3], R.f32(ref[3]))
        if n % 4 == 0:      # the other form on the same data
            other = be.col_stats(z, (n, 1) if form == P.FLOAT4 else None, P.SCALAR if form == P.FLOAT4 else P.FLOAT4)
            LEDGER.check("col_stats float4 against scalar", "sum", got[0], other[0], 2 * bound[0])
            LEDGER.check("col_stats float4 against scalar", "centred squares", got[1], other[1], 2 * bound[1])
            LEDGER.exact("col_stats float4 against scalar", "min / max", got[2:], other[2:])


@pytest.mark.parametrize("rows,family", COL_STATS_CASES)
def test_col_stats(be, rows, family):
    row_col_stats(be, rows, family)


FINALIZE_CASES = [(tiles, fam) for tiles in (0, 1, 2, 32, 33, 256, 257) for fam in ("base", "hetero", "offset")]      # tiles 0: rows == 1
FINALIZE_OPTIONS = [      # unbiased, momentum, moving buffers, with_range kind
    (True, 0.99, True, None), (False, 0.9, True, "none"), (True, 0.9, False, "relu"), (False, 0.99, True, "prelu")]


def row_bn_finalize(be, tiles, family):
    """col_stats + bn_finalize against the statistics of z in float64: tiles in {1, 2, 32, 33, 256, 257} with a ragged last tile of 44 rows (257:
    the second trip of a lane's loop, FIN_LANES * FIN_BATCH = 256 tiles a trip), rows == 1, n in {5, 8, 12} around FIN_CH = 8, unbiased on / off,
    momentum 0.9 / 0.99, no moving buffers, the range outputs without an activation, under ReLU and under a slope of both signs; channel 2 has
    a negative gamma.  The merge runs in double, so L is col_stats' 16 + 8; the cross term of the variance at a large mean and every
    later rounding: R.bn_finalize_truth.  zmin / zmax are exact, amax is the float32 formula on the kernel's own outputs, bit for bit."""
    rows = 1 if tiles == 0 else (tiles - 1) * R.TILE_M + 44
    assert R.tiles_of(rows) == max(tiles, 1) and P.finalize_trips(R.tiles_of(rows)) == (2 if tiles > 256 else 1)
    rs = np.random.RandomState(seed_of("finalize", tiles, family))
    for n in (5, 8, 12):
        z = R.make_z(rs, rows, n, family)
        gamma, beta = R.make_affine(rs, n, family, negative=2)
        part = be.col_stats(z, None, P.FLOAT4 if n % 4 == 0 else P.SCALAR)
        for unbiased, momentum, moving, rng in FINALIZE_OPTIONS:
            mm, mv = (R.f32(rs.randn(n)), R.f32(rs.rand(n) + 0.5)) if moving else (None, None)
            relu, slope, _ = slope_of(rs, rng or "relu", n)
            got = be.bn_finalize(part, rows, gamma, beta, EPS, momentum, unbiased, mm, mv, with_range=rng is not None, relu=relu, slope=slope)
            ref, bound = R.bn_finalize_truth(z, gamma, beta, EPS, momentum, unbiased, mm, mv)
            form = "bn_finalize%s" % (" (second trip)" if tiles > 256 else "")
            for key in bound:
                cap = family == "base" and rows > 1      # test_affine_forward_and_bn_stats of tests/test_gpu_ops.py: 1e-4 of the largest entry
                LEDGER.check(form, key, got[key], ref[key], LEDGER.capped(bound[key], ref[key], 1e-4) if cap else bound[key])
            if rng is not None:
                LEDGER.exact(form, "zmin", got["zmin"], R.f32(ref["zmin"]))
                LEDGER.exact(form, "zmax", got["zmax"], R.f32(ref["zmax"]))
                want = R.output_range_amax(got["zmin"], got["zmax"], got["scale"], got["shift"], relu, slope)
                LEDGER.exact(form, "amax (%s)" % rng, np.float32(got["amax"]), want)
                if rng == "prelu":
                    assert (got["scale"] < 0).any() and (got["scale"] > 0).any() and (slope < 0).any()


@pytest.mark.parametrize("tiles,family", FINALIZE_CASES)
def test_bn_finalize(be, tiles, family):
    row_bn_finalize(be, tiles, family)


OUTPUT_RANGE_CASES = [(tiles, kind) for tiles in (1, 3) for kind in ("none", "relu", "prelu")]


def row_bn_output_range(be, tiles, kind):
    """bn_output_range_kernel with scale and shift that are not the batch's own (the inference pair): zmin / zmax are the exact minimum and
    maximum of the column, amax is bit for bit the float32 formula on them (R.output_range_amax).  n = 12 and n = 130 (a second block of 128 threads)."""
    rows = (tiles - 1) * R.TILE_M + 44
    rs = np.random.RandomState(seed_of("range", tiles, kind))
    for n in (12, 130):
        z = R.make_z(rs, rows, n, "hetero")
        scale, shift = R.make_affine(rs, n, "hetero", negative=2)
        relu, slope, _ = slope_of(rs, kind, n)
        part = be.col_stats(z)
        zmin, zmax, amax = be.bn_output_range(part, rows, scale, shift, relu, slope)
        LEDGER.exact("bn_output_range", "zmin", zmin, z.min(axis=0))
        LEDGER.exact("bn_output_range", "zmax", zmax, z.max(axis=0))
        LEDGER.exact("bn_output_range", "amax (%s)" % kind, np.float32(amax), R.output_range_amax(z.min(axis=0), z.max(axis=0), scale, shift, relu, slope))


@pytest.mark.parametrize("tiles,kind", OUTPUT_RANGE_CASES)
def test_bn_output_range(be, tiles, kind):
    row_bn_output_range(be, tiles, kind)


def row_bn_inference_scale(be, n):
    """bn_inference_scale_kernel, n in {1, 128, 129} around its block of 128 threads; element-wise (R.bn_inference_scale_bound)."""
    rs = np.random.RandomState(seed_of("inference", n))
    gamma, beta = R.make_affine(rs, n, "hetero", negative=0)
    mm, mv = R.f32(rs.randn(n) * R.channel_scale(n)), R.f32((rs.rand(n) + 0.1) * R.channel_scale(n) ** 2)
    scale, shift = be.bn_inference_scale(gamma, beta, mm, mv, EPS)
    ref, (b_scale, b_shift) = R.bn_inference_scale(gamma, beta, mm, mv, EPS), R.bn_inference_scale_bound(gamma, beta, mm, mv, EPS)
    LEDGER.check("bn_inference_scale", "scale", scale, ref[0], b_scale)
    LEDGER.check("bn_inference_scale", "shift", shift, ref[1], b_shift)


@pytest.mark.parametrize("n", [1, 128, 129])
def test_bn_inference_scale(be, n):
    row_bn_inference_scale(be, n)


APPLY_CASES = [(kind, pitched) for kind in KINDS for pitched in (False, True)]


def row_bn_apply(be, kind, pitched):
    """bn_apply_kernel: rows in {1, 31, 32, 33} around its strip of 32 rows, n in {4, 256, 260} (n / 4 = 65: a second block of 64 column quads),
    input and output pitched by 4 and 8 floats; element-wise, 2 u (|z scale| + |shift|) and the slope (R.bn_apply_bound)."""
    rs = np.random.RandomState(seed_of("apply", kind, pitched))
    for rows in (1, 31, 32, 33):
        for n in (4, 256, 260):
            z = R.make_z(rs, rows, n, "hetero")
            scale, shift = R.make_affine(rs, n, "hetero", negative=1)
            relu, slope, _ = slope_of(rs, kind, n)
            got = be.bn_apply(z, scale, shift, relu, slope, ldz=n + 4 if pitched else None, lda=n + 8 if pitched else None)
            LEDGER.check("bn_apply%s" % (" pitched" if pitched else ""), kind, got, R.bn_apply(z, scale, shift, relu, slope),
                         R.bn_apply_bound(z, scale, shift, relu, slope))


@pytest.mark.parametrize("kind,pitched", APPLY_CASES)
def test_bn_apply(be, kind, pitched):
    row_bn_apply(be, kind, pitched)


# =========================================================================================== backward, fp32
def check_backward(be, form, row, got, red, z, gamma, mean, invstd, relu, slope, want_dalpha, segs=None, t=None, pad=0, residual=None, ceil=False):
    """The reductions against the float64 sums, dz against the float64 formula on the backend's own dgamma / dbeta (ambiguous elements left
    out), the pad frames exactly zero, dbias = gamma invstd (dbeta - fl(dbeta / rows) rows): zero up to 4 u |gamma invstd dbeta|."""
    r1, r2 = residual or (0.0, 0.0)
    dz_ref, b_dz = R.bn_backward_dz(red, z, gamma, mean, invstd, got["dbeta"], got["dgamma"])
    b_dbeta, b_dgamma, b_dalpha = red["b_dbeta"] + r1, red["b_dgamma"] + r2, red.get("b_dalpha")
    if ceil:      # the base family: the tolerances of test_bn_relu_backward / test_pooled_bn_backward_* of tests/test_gpu_ops.py as a ceiling
        b_dbeta, b_dgamma = LEDGER.capped(b_dbeta, red["dbeta"], 1e-4), LEDGER.capped(b_dgamma, red["dgamma"], 1e-4)
        b_dz = LEDGER.capped(b_dz, dz_ref, 2e-4)
        if want_dalpha:
            b_dalpha = LEDGER.capped(b_dalpha, red["dalpha"], 1e-4)
    LEDGER.check(form, "dbeta", got["dbeta"], red["dbeta"], b_dbeta)
    LEDGER.check(form, "dgamma", got["dgamma"], red["dgamma"], b_dgamma)
    if want_dalpha:
        LEDGER.check(form, "dalpha", got["dalpha"], red["dalpha"], b_dalpha)
    keep = ~red["ambiguous"]
    if segs is not None:
        dz_ref, b_dz, keep = R.pad_rows(dz_ref, segs, t, pad), R.pad_rows(b_dz, segs, t, pad), R.pad_rows(keep, segs, t, pad) | (R.pad_rows(b_dz, segs, t, pad) == 0)
    LEDGER.check(form, "dz", got["dz"], dz_ref, b_dz, keep)
    LEDGER.check(form, "dbias", got["dbias"], np.zeros(z.shape[1]),
                 4 * R.U * np.abs(R.f64(gamma) * R.f64(invstd)) * (np.abs(red["dbeta"]) + red["b_dbeta"] + r1) + 1e-300)
    note_share(form, row, red["ambiguous"])


PLAIN_SHAPES = [(1, r, 0) for r in (1, 63, 64, 65, 130)] + [(5, t, pad) for t in (1, 3, 31, 33) for pad in (2, 6)] + [(3, 31, 0), (3, 33, 0)]
PLAIN_CASES = [(kind, fam) for kind in KINDS for fam in ("base", "hetero")] + [("none", "offset")]


def row_plain_backward(be, kind, family, shapes=PLAIN_SHAPES, widths=(4, 256, 260)):
    """bn_bwd_reduce_kernel + bn_bwd_finalize_kernel + the apply pass (dense: pad == 0, strip: pad > 0, with segments of 1 and 3 frames shorter
    than a strip of 32 padded rows) through xv_bn_relu_backward: rows in {1, 63, 64, 65, 130} around the 64-row chunk, n in {4, 256, 260}.
    prelu: nstat 4 (dalpha), lrelu: a slope with nstat 3.  L = 16 + 2 + ceil(chunks / 32) + 32: a thread's 16 rows of the chunk in row
    order, (lane0 + lane1) + (lane2 + lane3), a finalize lane's chunks in order, the 32 lanes in lane order."""
    rs = np.random.RandomState(seed_of("plain", kind, family))
    for segs, t, pad in shapes:
        for n in widths:
            rows = segs * t
            if rows == 1 and family == "hetero":
                continue      # one row: the variance is 0 and y = beta only after z scale cancels against shift - at a channel scale of 1000 the
                              # rounding of that cancellation exceeds beta and every sign is ambiguous; the base family runs the shape
            z, da = R.make_z(rs, rows, n, family), R.make_grad(rs, (rows, n), family)
            gamma, beta = R.make_affine(rs, n, family, negative=1)
            relu, slope, want_dalpha = slope_of(rs, kind, n)
            plan = P.bn_bwd_plan(rows, pad=pad, relu=bool(relu), has_slope=slope is not None, has_dalpha=want_dalpha)
            assert plan == P.lib_bn_bwd_plan(rows, pad=pad, relu=bool(relu), has_slope=slope is not None, has_dalpha=want_dalpha)
            assert plan == (P.PLAIN_PASS, 0, 4 if kind == "prelu" else 3, R.cdiv(rows, 64), P.DENSE if pad == 0 else P.STRIP), plan
            mean, invstd, scale, shift = statistics(be, z, gamma, beta)
            got = be.bn_backward(z, gamma, mean, invstd, scale, shift, relu, slope, want_dalpha, da=da, segs=segs, t=t, pad=pad)
            L = R.PLAIN_BLOCK_L + R.finalize_chain(plan[3])
            red = R.bn_backward(z, gamma, mean, invstd, scale, shift, relu, slope, L, da=da)
            form = "plain backward %s, %s" % ("dense" if pad == 0 else "strip", "nstat 4" if plan[2] == 4 else "slope, nstat 3" if slope is not None else kind)
            check_backward(be, form, "plain %s %s %dx%dx%d pad %d" % (kind, family, segs, t, n, pad), got, red, z, gamma, mean, invstd, relu, slope,
                           want_dalpha, segs, t, pad, ceil=family == "base" and 63 <= rows <= 2048 and not red["ambiguous"].any())      # (the 16 385-row sum supplements no earlier row)
            if pad:
                dz = got["dz"].reshape(segs, t + 2 * pad, n)
                assert np.all(dz[:, :pad] == 0) and np.all(dz[:, pad + t:] == 0)


@pytest.mark.parametrize("kind,family", PLAIN_CASES)
def test_plain_backward(be, kind, family):
    row_plain_backward(be, kind, family)


@pytest.mark.parametrize("kind", KINDS)
def test_plain_backward_finalize_second_trip(be, kind):
    """rows = 16 385, n = 8: 257 chunks of 64 rows, the second trip of a lane's loop in bn_bwd_finalize_kernel (L = 16 + 2 + 9 + 32)."""
    assert P.finalize_trips(P.bn_bwd_plan(16385)[3]) == 2
    row_plain_backward(be, kind, "base", shapes=[(1, 16385, 0)], widths=(8,))


def pooled_inputs(rs, b, t, n, family, special):
    """z [b t][n], gamma, beta, d pool [b][2n].  special: chunk 0 constant (variance clamp; b >= 2), channel 1 off and channel 2 on for the whole
    last chunk (b >= 3), a negative gamma in channel 3."""
    z = R.make_z(rs, b * t, n, family).reshape(b, t, n)
    cs = R.channel_scale(n) if family == "hetero" else np.ones(n)
    if special and b >= 2:
        z[0] = z[0, :1]
    if special and b >= 3:
        z[b - 1, :, 1] = -50.0 * cs[1]
        z[b - 1, :, 2] = (50.0 + rs.rand(t)) * cs[2]
    gamma, beta = R.make_affine(rs, n, family, negative=3 if special else None)
    return R.f32(z.reshape(b * t, n)), gamma, beta, R.make_grad(rs, (b, 2 * n), family)


def frame_weights(rs, b, t, mode):
    """None | random positive weights summing to 1 | the same with the first min(5, t - 1) frames of every chunk exactly 0."""
    if mode is None:
        return None
    w = rs.rand(b, t) + 0.05
    if mode == "zeros":
        w[:, :min(5, t - 1)] = 0.0
    w = R.f32(w / w.sum(axis=1, keepdims=True))
    return w


DIRECT_CASES = [(kind, att, fam) for kind in ("none", "relu", "slope") for att in (False, True) for fam in ("base", "hetero")]


def row_pooled_direct(be, kind, att, family):
    """bn_bwd_reduce_pooled_kernel<RELU, HS, ATT>, all six instantiations (a slope: prelu with dalpha when weighted, lrelu otherwise), with T in
    {1, 31, 32, 33, 63, 64, 65, 129} - the apply pass turns from strip to dense at 32, nsub and rows_per change at 65 and 129 - b in {1, 3},
    n in {4, 260}.  L = 16 + 2 + ceil(chunks / 32) + 32 with chunks = b nsub: a thread's at most 16 rows of the block, the lane combine and the
    finalize kernel as in the plain pass.  The pooled statistics are the backend's own (float32) for the same activation."""
    rs = np.random.RandomState(seed_of("direct", kind, att, family))
    for t in (1, 31, 32, 33, 63, 64, 65, 129):
        for b in (1, 3):
            for n in (4, 260):
                if b * t == 1 and family == "hetero":
                    continue      # as in the plain pass: one row runs in the base family only
                z, gamma, beta, dpool = pooled_inputs(rs, b, t, n, family, special=False)
                relu, slope, want_dalpha = slope_of(rs, {"slope": "prelu" if att else "lrelu"}.get(kind, kind), n)
                w = frame_weights(rs, b, t, "random" if att else None)
                kw = dict(pooled=True, pool_t=t, relu=bool(relu), has_slope=slope is not None, has_dalpha=want_dalpha, has_weights=att)
                plan = P.bn_bwd_plan(b * t, **kw)
                assert plan == P.lib_bn_bwd_plan(b * t, **kw)
                flags = (P.RELU if relu else 0) | (P.HS if slope is not None else 0) | (P.ATT if att else 0)
                assert plan == (P.POOLED_PASS, flags, 4 if want_dalpha else 3, b * P.pooled_pass_geometry(t)[0], P.DENSE if t >= 32 else P.STRIP), plan
                mean, invstd, scale, shift = statistics(be, z, gamma, beta)
                pool = be.stat_pool_forward_bn(z, b, t, scale, shift, relu, slope, w, aux=False)
                got = be.bn_backward(z, gamma, mean, invstd, scale, shift, relu, slope, want_dalpha, pooled=(pool, dpool, t, w))
                L = R.POOLED_BLOCK_L + R.finalize_chain(plan[3])
                red = R.bn_backward(z, gamma, mean, invstd, scale, shift, relu, slope, L, pooled=(pool, dpool, t, w))
                form = "pooled pass <%d,%d,%d>, %s" % (bool(relu), slope is not None, att, "dense" if t >= 32 else "strip")
                check_backward(be, form, "direct %s att %d %s %dx%dx%d" % (kind, att, family, b, t, n), got, red, z, gamma, mean, invstd, relu, slope, want_dalpha,
                               ceil=family == "base" and b >= 3 and t >= 31 and not red["ambiguous"].any())      # (b == 1 without an activation: dz is 0 in exact arithmetic)


@pytest.mark.parametrize("kind,att,family", DIRECT_CASES)
def test_pooled_backward_direct_pass(be, kind, att, family):
    row_pooled_direct(be, kind, att, family)


CLOSED_CASES = [(relu, att, fam) for relu in (1, 0) for att in (False, True) for fam in ("base", "hetero")]


def row_pooled_closed(be, relu, att, family):
    """bn_bwd_pooled_stats_kernel (xv_bn_relu_backward_pooled_aux) with and without attention weights, under ReLU and without an activation
    (wpos == 1): b in {1, 63, 64, 65, 130} around PS_LANES = 64, n in {4, 16, 20} around a block's 16 channels, T in {31, 32, 33} around the
    strip / dense boundary; a constant chunk, a channel off and one on for a whole chunk, a negative gamma.  L = ceil(b / 64) + 64: a lane's
    chunks in order, then the 64 lanes in lane order; the kernel divides by gamma.  Three comparisons:
      - with its own formula in float64 on the float32 statistics it was handed (R.closed_form);
      - with the float64 sums over z it replaces, the bound widened by what the errors of those statistics can move (R.closed_form_residual,
        from the pooling row's bounds);
      - with the direct pass on the same input, within the sum of the two bounds - and dz of the dense kernel's affine shortcut with dz of
        its general branch (a slope vector of zeros: plain ReLU through the general code), within the sum of their bounds."""
    rs = np.random.RandomState(seed_of("closed", relu, att, family))
    for b in (1, 63, 64, 65, 130):
        for n in (4, 16, 20):
            for t in (31, 32, 33):
                z, gamma, beta, dpool = pooled_inputs(rs, b, t, n, family, special=True)
                w = frame_weights(rs, b, t, "random" if att else None)
                rows = b * t
                kw = dict(pooled=True, pool_t=t, relu=bool(relu), has_weights=att)
                plan = P.bn_bwd_plan(rows, has_wpos=True, **kw)
                assert plan == P.lib_bn_bwd_plan(rows, has_wpos=True, **kw) and plan[0] == P.CLOSED and plan[4] == (P.DENSE if t >= 32 else P.STRIP)
                mean, invstd, scale, shift = statistics(be, z, gamma, beta)
                pool, wpos, _ = be.stat_pool_forward_bn(z, b, t, scale, shift, relu, None, w, aux=True)
                got = be.bn_backward(z, gamma, mean, invstd, scale, shift, relu, pooled=(pool, dpool, t, w), wpos=wpos)
                form = "closed form%s%s" % (", weights" if att else "", "" if relu else ", no activation")
                ref1, ref2, b1, b2 = R.closed_form(pool, dpool, wpos, gamma, mean, invstd, scale, shift, rows)
                LEDGER.check(form + " against its formula", "dbeta", got["dbeta"], ref1, b1)
                LEDGER.check(form + " against its formula", "dgamma", got["dgamma"], ref2, b2)
                # against the sums over z
                direct_plan = P.bn_bwd_plan(rows, **kw)
                L = R.POOLED_BLOCK_L + R.finalize_chain(direct_plan[3])
                red = R.bn_backward(z, gamma, mean, invstd, scale, shift, relu, None, L, pooled=(pool, dpool, t, w))
                d_mean_p, d_std, d_wpos, _ = R.stat_pool_bn_bound(z, b, t, scale, shift, relu, None, w)
                res = R.closed_form_residual(pool, dpool, wpos, gamma, mean, scale, shift, d_mean_p, d_std, d_wpos, w)
                chain = dict(red, b_dbeta=b1, b_dgamma=b2)
                check_backward(be, form + " against the sums over z, " + ("dense" if t >= 32 else "strip"),
                               "closed relu %d att %d %s %dx%dx%d" % (relu, att, family, b, t, n), got, chain, z, gamma, mean, invstd, relu, None, False,
                               residual=res, ceil=family == "base" and b >= 3 and not red["ambiguous"].any())
                # against the direct pass
                direct = be.bn_backward(z, gamma, mean, invstd, scale, shift, relu, pooled=(pool, dpool, t, w))
                LEDGER.check(form + " against the direct pass", "dbeta", got["dbeta"], direct["dbeta"], chain["b_dbeta"] + res[0] + red["b_dbeta"])
                LEDGER.check(form + " against the direct pass", "dgamma", got["dgamma"], direct["dgamma"], chain["b_dgamma"] + res[1] + red["b_dgamma"])
                if relu and t >= 32:
                    zero_slope = np.zeros(n, np.float32)
                    assert P.bn_bwd_plan(rows, has_slope=True, **kw)[:2] == (P.POOLED_PASS, P.RELU | P.HS | (P.ATT if att else 0))
                    general = be.bn_backward(z, gamma, mean, invstd, scale, shift, relu, zero_slope, pooled=(pool, dpool, t, w))
                    LEDGER.exact("pooled pass <1,1,%d> with a zero slope against <1,0,%d>" % (att, att), "dbeta, dgamma",
                                 np.stack([general["dbeta"], general["dgamma"]]), np.stack([direct["dbeta"], direct["dgamma"]]))
                    dz_ref, b_dz = R.bn_backward_dz(red, z, gamma, mean, invstd, direct["dbeta"], direct["dgamma"])
                    LEDGER.check("dense pooled apply, general branch", "dz", general["dz"], dz_ref, b_dz, ~red["ambiguous"])
                    LEDGER.check("dense pooled apply, affine shortcut", "dz", direct["dz"], dz_ref, b_dz, ~red["ambiguous"])
                    LEDGER.check("dense pooled apply, affine shortcut against general branch", "dz", direct["dz"], general["dz"], 2 * b_dz,
                                 ~red["ambiguous"])


@pytest.mark.parametrize("relu,att,family", CLOSED_CASES)
def test_pooled_backward_closed_form(be, relu, att, family):
    row_pooled_closed(be, relu, att, family)


# =========================================================================================== pooling and l2_scaling
POOL_T = (1, 2, 3, 4, 5, 28, 29, 32, 33, 61, 64, 65)
POOL_CASES = [(kind, wmode, fam) for kind in ("none", "relu", "prelu") for wmode in (None, "random", "zeros") for fam in ("base", "hetero")]


def row_stat_pool_forward(be, kind, wmode, family):
    """stat_pool_fwd_kernel through xv_stat_pool_forward (no BatchNorm; unit weights only), xv_stat_pool_forward_bn and _aux: T in {1 ... 5, 28, 29, 32,
    33, 61, 64, 65} around the unrolled loop (t + 28 < T) and the four frame lanes, C in {4, 256, 260} (C / 4 = 65: a second block), three
    chunks of which chunk 0 is constant: its std is exactly the clamp value, with weights too.  Weights: none (1 / n through v_rcp_f32, one ulp),
    random, and random with the first five frames exactly 0 (the n > 0 guards).  L = ceil(T / 4) + 4: a frame lane's frames one after the
    other, one merge of its two chains, three of the lanes (R.stat_pool_bound).  wpos and amax per (chunk, channel)."""
    rs = np.random.RandomState(seed_of("pool", kind, wmode, family))
    b = 3
    clamp = np.sqrt(np.float32(1e-12))
    for t in POOL_T:
        for c in (4, 256, 260):
            z, gamma, beta, _ = pooled_inputs(rs, b, t, c, family, special=False)
            z = z.reshape(b, t, c)
            z[0] = z[0, :1]
            z = z.reshape(b * t, c)
            relu, slope, _ = slope_of(rs, kind, c)
            w = frame_weights(rs, b, t, wmode)
            if kind == "none" and wmode is None:
                got = be.stat_pool_forward(z.reshape(b, t, c))
                mean, sd, _ = R.stat_pool(z.reshape(b, t, c))
                d_mean, d_sd = R.stat_pool_bound(R.f64(z).reshape(b, t, c), 0.0)
                LEDGER.check("stat_pool_forward", "mean", got[:, :c], mean, d_mean)
                LEDGER.check("stat_pool_forward", "std", got[:, c:], sd, d_sd)
                LEDGER.exact("stat_pool_forward", "std of a constant chunk", got[0, c:], np.full(c, clamp))
            scale, shift = gamma, beta      # any affine map serves: the kernel is handed the two vectors
            out, wpos, amax = be.stat_pool_forward_bn(z, b, t, scale, shift, relu, slope, w, aux=True)
            plain = be.stat_pool_forward_bn(z, b, t, scale, shift, relu, slope, w, aux=False)
            form = "stat_pool_forward_bn %s%s" % (kind, {None: "", "random": ", weights", "zeros": ", weights with leading zeros"}[wmode])
            LEDGER.exact(form, "with and without the by-products", plain, out)
            mean, sd, wp_ref, am_ref = R.stat_pool_bn(z, b, t, scale, shift, relu, slope, w)
            d_mean, d_sd, d_wpos, d_amax = R.stat_pool_bn_bound(z, b, t, scale, shift, relu, slope, w)
            if family == "base" and t >= 28:      # test_pooling_fused_into_bn of tests/test_gpu_ops.py: 5e-5 of the largest entry; amax 2e-4
                top = np.concatenate([mean, sd], axis=1)
                d_mean, d_sd, d_amax = LEDGER.capped(d_mean, top, 5e-5), LEDGER.capped(d_sd, top, 5e-5), LEDGER.capped(d_amax, am_ref, 2e-4)
            LEDGER.check(form, "mean", out[:, :c], mean, d_mean)
            LEDGER.check(form, "std", out[:, c:], sd, d_sd)
            LEDGER.exact(form, "std of a constant chunk", out[0, c:], np.full(c, clamp))
            LEDGER.check(form, "wpos", wpos, wp_ref, d_wpos)
            LEDGER.check(form, "amax", amax, am_ref, d_amax)
            if relu:
                note_share(form, "pool %s %s %s %dx%d" % (kind, wmode, family, t, c), R.pre_activation(z, scale, shift)[2])


@pytest.mark.parametrize("kind,wmode,family", POOL_CASES)
def test_stat_pool_forward(be, kind, wmode, family):
    row_stat_pool_forward(be, kind, wmode, family)


POOL_BWD_CASES = [(3, 1, 4), (3, 1, 260), (3, 5, 4), (3, 5, 260), (3, 33, 4), (3, 33, 260), (8, 1025, 1024)]


def row_stat_pool_backward(be, b, t, c):
    """stat_pool_bwd_kernel: T in {1, 5, 33}, C in {4, 260}, chunk 0 constant (T = 1: every chunk), so its std sits at the clamp and only the mean
    path carries gradient; 8 x 1025 x 1024: 2 099 200 channel quads, just over the 8 192 x 256 a grid covers in one trip.  Element-wise,
    6 u (|dmean / T| + |k (x - mean)|)."""
    if b * t * (c // 4) > 8192 * 256:
        assert b * t * (c // 4) - 8192 * 256 < 4096
    rs = np.random.RandomState(seed_of("pool_bwd", b, t, c))
    x = R.make_z(rs, b * t, c, "hetero").reshape(b, t, c)
    x[0] = x[0, :1]
    dout = R.make_grad(rs, (b, 2 * c), "hetero")
    out = be.stat_pool_forward(x)
    assert np.all(out[0, c:] == np.sqrt(np.float32(1e-12)))
    dx = be.stat_pool_backward(x, out, dout)
    LEDGER.check("stat_pool_backward%s" % (" (grid stride)" if b * t * (c // 4) > 8192 * 256 else ""), "dx", dx, R.stat_pool_backward(x, out, dout),
                 R.stat_pool_backward_bound(x, out, dout))
    LEDGER.check("stat_pool_backward", "dx of a clamped chunk", dx[0], np.broadcast_to(R.f64(dout)[0, None, :c] / t, (t, c)),
                 2 * R.U * np.abs(R.f64(dout)[0, None, :c]) / t)


@pytest.mark.parametrize("b,t,c", POOL_BWD_CASES)
def test_stat_pool_backward(be, b, t, c):
    row_stat_pool_backward(be, b, t, c)


L2_CASES = [(rows, n) for rows in (1, 3, 4, 5) for n in (1, 63, 64, 65, 512)]


def row_l2_scaling(be, rows, n):
    """l2_scaling_fwd_kernel / l2_scaling_bwd_kernel (a wave per row, four rows per workgroup): rows in {1, 3, 4, 5}, n in {1, 63, 64, 65, 512}; an
    all-zero row (the k = 0 branch of the backward), a 1e-8 row (under the clamp) and a 100x row - with one row, each in turn - and, for
    n >= 2, a row whose float32 sum of squares is exactly the clamp value 1e-12f, where ss >= eps keeps the gradient of the norm
    (tf.maximum hands the gradient to its first argument on a tie).  L = ceil(n / 64) + 6: a lane's elements in order, six butterfly steps."""
    rs = np.random.RandomState(seed_of("l2", rows, n))
    variants = [("zero", "tiny", "big")] if rows >= 3 else [("zero",), ("tiny",), ("big",)]
    if n >= 2:
        variants.append(("threshold",))
    for special in variants:
        x, dy = R.f32(rs.randn(rows, n)), R.f32(rs.randn(rows, n))
        live = None
        for i, what in enumerate(special):
            if what == "zero":
                x[i] = 0
            elif what == "tiny":
                x[i] *= np.float32(1e-8)
            elif what == "big":
                x[i] *= np.float32(100)
            else:
                x[rows - 1] = R.l2_threshold_row(n)
                ss32 = (x.astype(np.float32) ** 2).sum(axis=1, dtype=np.float32)
                assert ss32[rows - 1] == R.L2_EPS32
                live = ((R.f64(x) ** 2).sum(axis=1, keepdims=True) >= float(R.L2_EPS32))
                live[rows - 1] = True
        y = be.l2_scaling_forward(x, 30.0)
        y_ref = R.l2_scaling(x, 30.0)[0]
        LEDGER.check("l2_scaling forward", "y", y, y_ref, LEDGER.capped(R.l2_scaling_bound(x, 30.0), y_ref, 1e-5))      # test_l2_scaling of tests/test_gpu_ops.py: 1e-5
        dx = be.l2_scaling_backward(x, dy, 30.0)
        form = "l2_scaling backward%s" % (", sum of squares on the threshold" if special == ("threshold",) else "")
        LEDGER.check(form, "dx", dx, R.l2_scaling_backward(x, dy, 30.0, live), R.l2_scaling_backward_bound(x, dy, 30.0, live))


@pytest.mark.parametrize("rows,n", L2_CASES)
def test_l2_scaling(be, rows, n):
    row_l2_scaling(be, rows, n)
