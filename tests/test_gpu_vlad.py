"""Every entry point of csrc/xv_vlad.hip against the float64 restatement of tests/vlad_ref.py on the same float32 inputs, per element within the
bound derived there (the normalisation backward: vlad_ref.close_to_f32_eval), at the shapes at which a kernel can go wrong: 8 and 1 500 columns
(one partly filled wave of column quads / six column blocks), cluster counts below, on and over the kernels' groups of 8 (1, 3 + 2, 10 + 2,
17 + 3, 60 + 4) and off the multiple of 4 the GEMM pitch has, 1 / 7 / 8 / 9 / 200 frames (fewer frames than frame lanes, the four-frame row
blocks of the backward, the unrolled loop of the forward), 1 and 3 chunks.  Every result buffer has NaN behind it, which must still be there;
the logits' padding columns hold NaN, which must not reach the softmax.  $XV_BOUNDS_OUT names a file that receives the largest ratio to its
bound per entry point."""
import atexit
import os

import numpy as np
import pytest

import vlad_ref as V

pytestmark = pytest.mark.gpu

WORST = {}


def note(name, err, bound):
    ratio = float(np.max(err / np.where(bound > 0, bound, 1.0))) if np.size(err) else 0.0
    WORST[name] = max(WORST.get(name, 0.0), ratio)
    bad = np.argwhere(err > bound)
    assert bad.size == 0, "%s: %d elements outside the bound, first %s: error %.3g, bound %.3g" % (
        name, len(bad), tuple(bad[0]), err[tuple(bad[0])], bound[tuple(bad[0])])


def note_ratio(name, ok, ratio, detail):
    WORST[name] = max(WORST.get(name, 0.0), ratio)
    assert ok, "%s: %.3g of the allowance (per chunk: error, the float32 evaluation's own, allowance) %s" % (name, ratio, detail)


@atexit.register
def _write_ledger():
    path = os.environ.get("XV_BOUNDS_OUT")
    if path and WORST:
        with open(path, "a") as f:
            f.write("# vlad entry points: largest error / bound over tests/test_gpu_vlad.py (normalize_backward: / 8 x the float32 NumPy evaluation's own distance)\n")
            for name in sorted(WORST):
                f.write("%-28s %.4f\n" % (name, WORST[name]))


class Gpu(object):
    def __init__(self):
        import torch
        from tf_kaldi_speaker_amd import _lib, ops
        self.torch, self.lib, self.ops = torch, _lib, ops

    def up(self, a, dtype=np.float32):
        return self.torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to("cuda")

    def out(self, *shape):
        n = int(np.prod(shape))
        buf = self.torch.full((n + 4,), float("nan"), dtype=self.torch.float32, device="cuda")
        return buf, shape

    def done(self, res, what):
        buf, shape = res
        h = buf.cpu().numpy()
        n = int(np.prod(shape))
        assert np.all(np.isnan(h[n:])), "%s wrote beyond its result" % what
        return h[:n].reshape(shape).copy()

    def call(self, name, *args):
        p, s = self.ops._p, self.ops._s()
        self.lib.call(name, s, *[p(a[0]) if isinstance(a, tuple) else (p(a) if (a is None or hasattr(a, "data_ptr")) else a) for a in args])

    # NumPy in, NumPy out
    def softmax(self, logits_padded, kg):
        rows, ld = logits_padded.shape
        d, res = self.up(logits_padded), self.out(rows, kg)
        self.call("xv_vlad_softmax", d, rows, kg, ld, res)
        return self.done(res, "xv_vlad_softmax")

    def pool_forward(self, x, a, cen, k, frames=None, shrink=0):
        b, t, c = x.shape
        kg = cen.shape[0]
        dx, da, dc = self.up(x), self.up(a), self.up(cen)
        df = None if frames is None else self.up(frames, np.int32)
        r, n = self.out(b, k, c), self.out(b, k)
        self.call("xv_vlad_pool_forward", dx, da, dc, b, t, c, k, kg, df, int(shrink), r, n)
        return self.done(r, "xv_vlad_pool_forward (r)"), self.done(n, "xv_vlad_pool_forward (n)")

    def normalize_forward(self, r, final):
        b, k, c = r.shape
        d, res = self.up(r), self.out(b, k * c)
        self.call("xv_vlad_normalize_forward", d, b, k, c, int(final), res)
        return self.done(res, "xv_vlad_normalize_forward")

    def normalize_backward(self, r, dout, final):
        b, k, c = r.shape
        d, g, res = self.up(r), self.up(dout), self.out(b, k, c)
        self.call("xv_vlad_normalize_backward", d, g, b, k, c, int(final), res)
        return self.done(res, "xv_vlad_normalize_backward")

    def pool_backward(self, x, a, cen, dr):
        b, t, c = x.shape
        k, kg = dr.shape[1], cen.shape[0]
        d_x, d_a, d_c, d_r = self.up(x), self.up(a), self.up(cen), self.up(dr)
        da, dx = self.out(b * t, kg), self.out(b, t, c)
        self.call("xv_vlad_pool_backward", d_x, d_a, d_c, d_r, b, t, c, k, kg, da, dx)
        return self.done(da, "xv_vlad_pool_backward (da)"), self.done(dx, "xv_vlad_pool_backward (dx)")

    def softmax_backward(self, a, da, ld):
        rows, kg = a.shape
        d_a, d_g, res = self.up(a), self.up(da), self.out(rows, ld)
        self.call("xv_vlad_softmax_backward", d_a, d_g, rows, kg, ld, res)
        return self.done(res, "xv_vlad_softmax_backward")

    def centers_backward(self, n, dr, cen, l2):
        b, k, c = dr.shape
        kg = cen.shape[0]
        d_n, d_r, d_c, res = self.up(n), self.up(dr), self.up(cen), self.out(kg, c)
        self.lib.call("xv_vlad_centers_backward", self.ops._s(), self.ops._p(d_n), self.ops._p(d_r), self.ops._p(d_c), b, k, kg, c, float(l2), self.ops._p(res[0]))
        return self.done(res, "xv_vlad_centers_backward")


@pytest.fixture(scope="module")
def gpu():
    return Gpu()


def padded_logits(x, w, bias):
    """float32 logits [rows, kg] inside a [rows, pitch4(kg)] buffer whose padding columns are NaN."""
    b, t, c = x.shape
    kg = w.shape[1]
    lg = V.f32(V.f64(x).reshape(b * t, c) @ V.f64(w) + V.f64(bias))
    buf = np.full((b * t, (kg + 3) // 4 * 4), np.nan, np.float32)
    buf[:, :kg] = lg
    return lg, buf


def check_all(gpu, x, w, bias, cen, k, rs, tag):
    """Every entry point on one case; each stage takes the float32 rounding of the float64 result of the stage before, on both sides."""
    b, t, c = x.shape
    kg = cen.shape[0]
    lg, buf = padded_logits(x, w, bias)
    a = gpu.softmax(buf, kg)
    note("softmax", np.abs(a - V.softmax(lg)), V.softmax_bound(lg))
    a = V.f32(V.softmax(lg))
    r, n = gpu.pool_forward(x, a, cen, k)
    r64, n64 = V.pool_forward(x, a, cen, k)
    br, bn = V.pool_forward_bound(x, a, cen, k)
    note("pool_forward r", np.abs(r - r64), br)
    note("pool_forward n", np.abs(n - n64), bn)
    r, n = V.f32(r64), V.f32(n64)
    dout = V.f32(rs.randn(b, k * c))
    for final in (False, True):
        out = gpu.normalize_forward(r, final)
        note("normalize_forward", np.abs(out - V.normalize_forward(r, final)), V.normalize_forward_bound(r, final))
        dr = gpu.normalize_backward(r, dout, final)
        assert np.all(np.isfinite(dr)), tag
        ok, ratio, detail = V.close_to_f32_eval(dr, V.normalize_backward(r, dout, final), V.normalize_backward(r, dout, final, np.float32))
        note_ratio("normalize_backward", ok, ratio, detail)
    dr = V.f32(rs.randn(b, k, c))
    da, dx = gpu.pool_backward(x, a, cen, dr)
    da64, dx64 = V.pool_backward(x, a, cen, dr)
    bda, bdx = V.pool_backward_bound(x, a, cen, dr)
    note("pool_backward da", np.abs(da - da64), bda)
    note("pool_backward dx", np.abs(dx - dx64), bdx)
    assert np.all(da[:, k:] == 0), "%s: a ghost cluster received a gradient from the pooling" % tag
    da = V.f32(da64)
    ld = (kg + 3) // 4 * 4
    dl = gpu.softmax_backward(a, da, ld)
    note("softmax_backward", np.abs(dl[:, :kg] - V.softmax_backward(a, da)), V.softmax_backward_bound(a, da))
    assert np.all(dl[:, kg:] == 0), "%s: the padding columns of d logits must be zero" % tag
    dc = gpu.centers_backward(n, dr, cen, 0.01)
    note("centers_backward", np.abs(dc - V.centers_backward(n, dr, cen, 0.01)), V.centers_backward_bound(n, dr, cen, 0.01))
    assert np.all(dc[k:] == np.float32(0.01) * cen[k:]), "%s: a ghost centre has only the regulariser's gradient" % tag


@pytest.mark.parametrize("b", [1, 3])
@pytest.mark.parametrize("t", [1, 7, 8, 9, 200])
@pytest.mark.parametrize("kg", [(1, 0), (3, 2), (10, 2), (17, 3), (60, 4)])
@pytest.mark.parametrize("c", [8, 1500])
def test_entry_points_against_float64(gpu, c, kg, t, b):
    k, g = kg
    rs = np.random.RandomState(1000 * b + 10 * t + c + k)
    x, w, bias, cen = V.make_case(rs, b, t, c, k, g)
    check_all(gpu, x, w, bias, cen, k, rs, "c=%d k=%d g=%d t=%d b=%d" % (c, k, g, t, b))


@pytest.mark.parametrize("c", [24, 1500])
def test_hostile_chunks_of_the_reference_self_test(gpu, c):
    """model/pooling.py:478-510: a chunk times 1e-8, a zero chunk, a chunk times 100, the constant 100 - 10 + 2 clusters; nothing is NaN."""
    rs = np.random.RandomState(c)
    x, w, bias, cen = V.make_case(rs, 4, 13, c, 10, 2, hostile=True)
    check_all(gpu, x, w, bias, cen, 10, rs, "hostile c=%d" % c)


@pytest.mark.parametrize("final", [False, True])
def test_zero_residual_is_zero_with_finite_gradients(gpu, final):
    """Every frame equals every centre: R is exactly 0, so is the output, and the gradient passes the clamped norm as 1 / sqrt(eps)."""
    b, t, c, k, g = 2, 9, 1500, 3, 2
    rs = np.random.RandomState(5)
    cen = np.tile(V.f32(rs.rand(c)), (k + g, 1))
    x = np.tile(cen[0], (b, t, 1))
    a = V.f32(V.softmax(rs.randn(b * t, k + g)))
    r, n = gpu.pool_forward(x, a, cen, k)
    assert np.all(r == 0)
    assert np.all(gpu.normalize_forward(r, final) == 0)
    dout = V.f32(rs.randn(b, k * c))
    dr = gpu.normalize_backward(r, dout, final)
    want = V.normalize_backward(r, dout, final)
    assert np.all(np.isfinite(dr)) and np.all(np.abs(dr - want) <= 8 * V.RSQRT_REL * np.abs(want))      # two rsqrt of the epsilon, three products
    da, dx = gpu.pool_backward(x, a, cen, V.f32(dr))
    assert np.all(np.isfinite(da)) and np.all(np.isfinite(dx)) and np.all(da == 0)      # x - c is exactly 0


def test_ragged_frames_with_shrink(gpu):
    """Batched extraction (the contract of xv_stat_pool_forward_bn_ex): chunk i pools its first frames[i] - shrink rows; the rows behind hold
    NaN here, so a kernel that read them would show it."""
    b, t, c, k, g, shrink = 4, 23, 1500, 10, 2, 14
    rs = np.random.RandomState(9)
    x, w, bias, cen = V.make_case(rs, b, t, c, k, g)
    frames = np.array([t + shrink, 15, 26, 30])       # 23, 1, 12 and 16 valid rows
    a = V.f32(V.softmax(rs.randn(b * t, k + g)))
    xn = x.copy()
    for i, tv in enumerate(V.valid_frames(t, frames, shrink)):
        xn[i, tv:] = np.nan
    r, n = gpu.pool_forward(xn, a, cen, k, frames, shrink)
    r64, n64 = V.pool_forward(x, a, cen, k, frames, shrink)
    br, bn = V.pool_forward_bound(x, a, cen, k, frames, shrink)
    note("pool_forward r (ragged)", np.abs(r - r64), br)
    note("pool_forward n (ragged)", np.abs(n - n64), bn)


@pytest.mark.parametrize("b", [16, 17, 37])
def test_centers_backward_over_many_chunks(gpu, b):
    """The chunk lanes of vlad_centers_bwd_kernel: one chunk per lane, one lane with a second chunk, three trips with idle lanes in the last."""
    c, k, g = 24, 3, 2
    rs = np.random.RandomState(b)
    cen = V.f32(rs.randn(k + g, c) * 0.1)
    n, dr = V.f32(rs.rand(b, k) * 20), V.f32(rs.randn(b, k, c))
    dc = gpu.centers_backward(n, dr, cen, 0.01)
    note("centers_backward", np.abs(dc - V.centers_backward(n, dr, cen, 0.01)), V.centers_backward_bound(n, dr, cen, 0.01))


def test_repitch_pads_with_zeros_and_drops_padding(gpu):
    rs = np.random.RandomState(0)
    w = V.f32(rs.randn(1500, 10))
    d_w, res = gpu.up(w), gpu.out(1500, 12)
    gpu.call("xv_vlad_repitch", d_w, 1500, 10, 10, res, 12)
    wp = gpu.done(res, "xv_vlad_repitch")
    assert np.array_equal(wp[:, :10], w) and not wp[:, 10:].any()
    d_p, back = gpu.up(wp), gpu.out(1500, 10)
    gpu.call("xv_vlad_repitch", d_p, 1500, 10, 12, back, 10)
    assert np.array_equal(gpu.done(back, "xv_vlad_repitch"), w)
    assert np.array_equal(gpu.ops.vlad_repitch(gpu.up(w[:3]), 12).cpu().numpy(), wp[:3])


def test_two_calls_give_the_same_bits(gpu):
    b, t, c, k, g = 3, 200, 1500, 10, 2
    rs = np.random.RandomState(77)
    x, w, bias, cen = V.make_case(rs, b, t, c, k, g)
    lg, buf = padded_logits(x, w, bias)
    dout, dr0 = V.f32(rs.randn(b, k * c)), V.f32(rs.randn(b, k, c))

    def run():
        a = gpu.softmax(buf, k + g)
        r, n = gpu.pool_forward(x, a, cen, k)
        out = gpu.normalize_forward(r, True)
        dr = gpu.normalize_backward(r, dout, True)
        da, dx = gpu.pool_backward(x, a, cen, dr0)
        dl = gpu.softmax_backward(a, da, 12)
        dc = gpu.centers_backward(n, dr0, cen, 0.01)
        return [a, r, n, out, dr, da, dx, dl, dc]
    for u, v in zip(run(), run()):
        assert u.tobytes() == v.tobytes()


def test_wrappers_check_their_arguments(gpu):
    torch, ops = gpu.torch, gpu.ops
    x = torch.zeros(2, 3, 8, device="cuda")
    a = torch.zeros(6, 5, device="cuda")
    cen = torch.zeros(5, 8, device="cuda")
    r, n = ops.vlad_pool_forward(x, a, cen, 3)
    assert tuple(r.shape) == (2, 3, 8) and tuple(n.shape) == (2, 3)
    with pytest.raises(ValueError, match="1 <= centers 6 <= clusters 5 <= 64"):
        ops.vlad_pool_forward(x, a, cen, 6)
    with pytest.raises(ValueError, match="the assignment weights"):
        ops.vlad_pool_forward(x, a[:5], cen, 3)
    with pytest.raises(ValueError, match="multiple of 4"):
        ops.vlad_pool_forward(torch.zeros(2, 3, 6, device="cuda"), a, torch.zeros(5, 6, device="cuda"), 3)
    with pytest.raises(ValueError, match="clusters 65"):
        ops.vlad_softmax(torch.zeros(4, 68, device="cuda"), 65)
    with pytest.raises(gpu.lib.XvError, match="vlad_pool_forward: bad arguments"):
        gpu.lib.call("xv_vlad_pool_forward", ops._s(), ops._p(x), ops._p(a), ops._p(cen), 2, 3, 8, 6, 5, None, 0, ops._p(r), ops._p(n))
