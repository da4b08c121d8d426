"""Every form of the split-precision (f16x3) kernels of csrc/xv_planes16.hip, xv_gemm16_nt.hip and xv_gemm16_tn.hip - the plane emitters, the generic and the context-window NT
kernels with their epilogues, the TN weight-gradient kernel with its stage forms - at the smallest shapes that reach it.  A row first
asserts its form through the restatement of tests/test_gemm16_plans.py and the library's hook, so a row that drifts to another branch
fails by name.  A GEMM row then runs twice: on position-coded integer operands (every piece, product and partial sum exactly representable:
the result must equal the float64 result bit for bit, whatever row, tap, chunk, swizzle or tile went wrong) and on random operands
against the bound derived in tests/gemm16_ref.py, per element.  The planes of the emitters are compared with the model bit for bit.

Results go into NaN-surrounded pitched buffers whose pads must still be NaN afterwards, the weight-gradient workspace is exactly as large
as the plan needs and filled with NaN before each launch.  The rows are functions of a backend; tests/test_gemm16_ref.py hands them a
plain float32 NumPy evaluation first.  The 256-row tiles of the context-window kernel are read from XV_CONV_WR once per process: their
rows (defined only in such a process) run in one child.  $XV_BOUNDS_OUT names a file that receives the largest ratio to its bound per form
and the wall time of the module."""
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import bn_pool_ref as R
import gemm16_ref as S
import test_gemm16_plans as P
import test_gpu_attention_forms as GA
import test_gpu_bn_pool_forms as G
from test_gpu_bn_pool_forms import seed_of, slope_of

pytestmark = pytest.mark.gpu

CONV_WR = 4 if os.environ.get("XV_CONV_WR") == "4" else 0
LEDGER = R.Ledger()
SHARES = {}
SENTINEL = 0x7e7e      # an fp16 NaN around the planes


def note_share(form, row, amb):
    share = float(np.mean(amb)) if amb.size else 0.0
    SHARES[form] = max(SHARES.get(form, 0.0), share)
    assert share <= R.MAX_AMBIGUOUS_SHARE, "%s: %.3g of the elements are mask-ambiguous (cap %.0e): change the seed" % (row, share, R.MAX_AMBIGUOUS_SHARE)


def write_ledger(tag, seconds):
    G.write_ledger(tag, seconds, LEDGER, SHARES, "gemm16 forms%s" % (", 256-row tiles" if CONV_WR == 4 else ""))
    LEDGER.worst.clear()      # (also without $XV_BOUNDS_OUT: the CPU module of these rows shares this ledger)
    SHARES.clear()


class GpuOps(GA.GpuOps):
    """float32 NumPy in, NumPy out, through the C entry points on buffers of this class."""

    def bits(self, value):
        return self.torch.tensor([value if value < (1 << 31) else value - (1 << 32)], dtype=self.torch.int32, device=self.dev_name)

    def planes_out(self, rows, ld):
        buf = self.torch.full((2 * rows * ld + 16,), SENTINEL, dtype=self.torch.int16, device=self.dev_name)
        return buf, buf[:2 * rows * ld]

    def planes_done(self, buf, rows, ld, what):
        h = self.host(buf).view(np.uint16)
        assert np.all(h[2 * rows * ld:] == SENTINEL), "%s wrote beyond its planes" % what
        return h[:2 * rows * ld].reshape(2, rows, ld).copy()

    # ---- emitters
    def amax(self, x, prev=0, offset=0):
        flat = np.ravel(x)
        src = self.view(flat[None, :], None, offset)[0]
        a = self.bits(prev)
        self.lib.call("xv_amax", self.stream(), self.ops._p(src), C.c_size_t(flat.size), self.ops._p(a))
        return int(self.host(a).view(np.uint32)[0])

    def split(self, x, bits, lds=None, offset=0):
        rows, c = x.shape
        ld = P.align8(c)
        src, a = self.view(x, lds, offset), self.bits(bits)
        buf, data = self.planes_out(rows, ld)
        self.lib.call("xv_split_planes", self.stream(), self.ops._p(src), rows, c, src.stride(0), self.ops._p(data), ld, C.c_size_t(rows * ld),
                      self.ops._p(a))
        return self.planes_done(buf, rows, ld, "xv_split_planes")

    def bn_apply_split(self, z, scale, shift, relu, slope, bits, ldz=None):
        rows, n = z.shape
        ld = P.align8(n)
        src, d_scale, d_shift, a = self.view(z, ldz), self.vec(scale), self.vec(shift), self.bits(bits)
        buf, data = self.planes_out(rows, ld)
        with self.activation(slope):
            self.lib.call("xv_bn_apply_split", self.stream(), self.ops._p(src), rows, n, src.stride(0), self.ops._p(d_scale), self.ops._p(d_shift),
                          int(relu), self.ops._p(a), self.ops._p(data), ld, C.c_size_t(rows * ld))
        return self.planes_done(buf, rows, ld, "xv_bn_apply_split")

    # ---- GEMMs
    def operand(self, a2):
        """Planes of a [rows][c] matrix as the device emitters make them (their own rows check them) -> (Planes, amax bits)"""
        p = self.ops.split_planes(self.dev(a2))
        return p, int(self.host(p.amax).view(np.uint32)[0])

    def result(self, rows, n, ld):
        return self.torch.full(((rows + 2) * ld,), float("nan"), dtype=self.torch.float32, device=self.dev_name)

    def collect(self, buf, rows, n, ld, what):
        full = self.host(buf).reshape(rows + 2, ld)
        c = full[:rows, :n].copy()
        full[:rows, :n] = np.nan
        assert np.all(np.isnan(full)), "%s wrote outside its %d x %d view (pitch %d)" % (what, rows, n, ld)
        return c

    def forward(self, x, kern, bias, stats=False, ldz=None, conv_wr=0):
        assert conv_wr == CONV_WR, "this process runs XV_CONV_WR=%d" % CONV_WR
        p = self.ops._p
        segs, t_in, c = x.shape
        k, _, o = kern.shape
        xp, ax = self.operand(x.reshape(-1, c))
        wtp, aw = self.operand(S.weights_fwd(kern, xp.ld))
        rows, ldz = segs * (t_in - k + 1), ldz or o
        tiles = R.tiles_of(rows)
        zbuf, d_bias = self.result(rows, o, ldz), self.vec(bias)
        pbuf, part = self.out(4 * tiles * o) if stats else (None, None)
        self.lib.call("xv_affine_forward_f16x3", self.stream(), p(xp.data), C.c_size_t(xp.stride), p(xp.amax), segs, t_in, xp.ld, k, p(wtp.data),
                      C.c_size_t(wtp.stride), p(wtp.amax), p(d_bias), p(zbuf), o, ldz, p(part))
        z = self.collect(zbuf, rows, o, ldz, "xv_affine_forward_f16x3")
        part = self.done(pbuf, 4 * tiles * o, "xv_affine_forward_f16x3 (statistics)").reshape(4, tiles, o) if stats else None
        return dict(z=z, part=part, ax=ax, aw=aw)

    def dgrad(self, dz, kern, bwd=None, conv_wr=0):
        assert conv_wr == CONV_WR, "this process runs XV_CONV_WR=%d" % CONV_WR
        p = self.ops._p
        segs, t_out, o = dz.shape
        k, c, _ = kern.shape
        dzp, adz = self.operand(S.padded(dz, k - 1).reshape(-1, o))
        wfp, aw = self.operand(S.weights_dgrad(kern, dzp.ld))
        rows = segs * (t_out + k - 1)
        tiles = R.tiles_of(rows)
        xbuf = self.result(rows, c, c)
        head = (self.stream(), p(dzp.data), C.c_size_t(dzp.stride), p(dzp.amax), segs, t_out, dzp.ld, k, p(wfp.data), C.c_size_t(wfp.stride),
                p(wfp.amax), p(xbuf), c)
        part = None
        if bwd is None:
            self.lib.call("xv_affine_dgrad_f16x3", *head)
        else:
            d_z = self.view(bwd["z"])
            vecs = [self.vec(bwd[key]) for key in ("scale", "shift", "mean", "invstd")]
            pbuf, d_part = self.out(tiles * 3 * c)
            self.lib.call("xv_affine_dgrad_bnstats_f16x3", *(head + (p(d_z),) + tuple(p(v) for v in vecs) + (p(d_part),)))
            part = self.done(pbuf, tiles * 3 * c, "xv_affine_dgrad_bnstats_f16x3 (partials)").reshape(tiles, 3, c)
        return dict(dx=self.collect(xbuf, rows, c, c, "xv_affine_dgrad_f16x3"), part=part, adz=adz, aw=aw)

    def wgrad(self, x, dz, kern, l2, pad=None, ws_short=0):
        p = self.ops._p
        segs, t_in, c = x.shape
        k, _, o = kern.shape
        t_out = t_in - k + 1
        pad = k - 1 if pad is None else pad
        xp, ax = self.operand(x.reshape(-1, c))
        dzp, adz = self.operand(S.padded(dz, pad).reshape(-1, o))
        m, n = k * xp.ld, dzp.ld
        splits = P.tn_plan(m, n, segs * t_out, t_out, t_in, t_out + 2 * pad)[1]
        ws = self.torch.full((splits * m * n,), float("nan"), dtype=self.torch.float32, device=self.dev_name)      # what the plan needs, not a float more
        kbuf, dk = self.out(k * c * o)
        d_kern = self.dev(kern)
        self.lib.call("xv_affine_wgrad_f16x3", self.stream(), p(xp.data), C.c_size_t(xp.stride), p(xp.amax), segs, t_in, xp.ld, k, c, p(dzp.data),
                      C.c_size_t(dzp.stride), p(dzp.amax), t_out + 2 * pad, pad, dzp.ld, o, p(d_kern), float(l2), p(dk), p(ws),
                      C.c_size_t(ws.numel() * 4 - ws_short))
        return dict(dk=self.done(kbuf, k * c * o, "xv_affine_wgrad_f16x3").reshape(k, c, o), ax=ax, adz=adz)


@pytest.fixture(scope="module")
def be():
    t0 = time.time()
    yield GpuOps()
    write_ledger("gpu", time.time() - t0)


# =========================================================================================== emitters
AMAX_CASES = [1, 3, 4, 5, 1024 * 256 * 4 + 5]      # the scalar tail alone, one quad, quad + tail, every block a second trip of the grid stride


def row_amax(be, count):
    """xv_amax: the quad loop and its count % 4 tail, the scalar branch of a source 4 bytes off 16-byte alignment, the 1024-block grid stride;
    the maximum in the last tail element and negative; accumulation onto a larger and onto a smaller previous value; bit equality."""
    rs = np.random.RandomState(seed_of("amax", count))
    x = R.f32(rs.randn(count) * 1e-3)
    x[-1] = -7.25
    for offset in (0, 1):
        form = "amax, %s" % ("quads" if offset == 0 else "scalar")
        got = be.amax(x, 0, offset)
        LEDGER.exact(form, "negative maximum in the last element", got, S.bits_of(7.25))
        LEDGER.exact(form, "the model", got, S.amax_bits(x))
        LEDGER.exact(form, "onto a larger value", be.amax(x, S.bits_of(8.0), offset), S.bits_of(8.0))
        LEDGER.exact(form, "onto a smaller value", be.amax(x, S.bits_of(7.0), offset), S.bits_of(7.25))
    if count > 4:
        x[-1], x[count // 2] = 0.5, 3.5
        LEDGER.exact("amax, quads", "maximum in the body", be.amax(x), S.bits_of(3.5))


@pytest.mark.parametrize("count", AMAX_CASES)
def test_amax(be, count):
    row_amax(be, count)


SPLIT_C = (1, 4, 7, 8, 12, 30, 1500)
SPLIT_LAYOUTS = [("contiguous", 0, 0), ("pitch % 4 = 0", 4, 0), ("pitch % 4 = 2", 6, 0), ("misaligned", 0, 1)]      # name, floats added to the pitch, base offset


def split_vec(c, lds, offset):
    return c % 4 == 0 and lds % 4 == 0 and offset % 4 == 0


def row_split_planes(be, c, scale):
    """xv_split_planes at c in {1, 4, 7, 8, 12, 30, 1500}: the float4 form (c % 4 == 0, pitch % 4 == 0, aligned source) and the scalar form
    behind each of its three conditions; scales 1e-7, 1, 1e3 with an outlier 1e4 times the typical value setting the scale (most low pieces
    are then subnormal fp16 or zero).  Both planes and every pad column bit for bit against the model."""
    rs = np.random.RandomState(seed_of("split", c, scale))
    rows = 37
    x = R.f32(rs.randn(rows, c) * scale)
    x[3, min(5, c - 1)] = 1e4 * scale
    bits = S.amax_bits(x)
    want = S.split(x, bits)
    assert np.all(want[:, :, c:] == 0)
    for name, extra, offset in SPLIT_LAYOUTS:
        form = "split planes, %s" % ("float4" if split_vec(c, c + extra, offset) else "scalar")
        LEDGER.exact(form, "planes (%s)" % name, be.split(x, bits, c + extra, offset), want)
    h, l = S.plane_values(want)
    rec = (R.f64(h) + R.f64(l))[:, :c] / float(S.pow2_scale(bits))
    LEDGER.check("split planes, model", "h + l against x", rec, x, S.eps_rep(x, bits))


@pytest.mark.parametrize("c", SPLIT_C)
@pytest.mark.parametrize("scale", [1e-7, 1.0, 1e3])
def test_split_planes(be, c, scale):
    row_split_planes(be, c, scale)


def row_split_planes_special(be):
    """An all-zero tensor (amax = 0: scale 1, planes 0), an amax far above the data (everything lands in the low plane's subnormals or
    vanishes), and one tensor of 8192 x 256 + 3 chunks: a second trip of the grid-stride loop."""
    z = np.zeros((4, 8), np.float32)
    LEDGER.exact("split planes, float4", "all zero", be.split(z, S.amax_bits(z)), np.zeros((2, 4, 8), np.uint16))
    rs = np.random.RandomState(seed_of("split special"))
    x = R.f32(rs.randn(37, 30))
    for bits in (S.bits_of(2.0 ** 30), S.bits_of(np.inf), S.bits_of(2.0 ** -120)):
        if S.pow2_scale(bits) * np.abs(x).max() < 6e4:      # (an amax below the data would overflow fp16: not a state the producers reach)
            LEDGER.exact("split planes, scalar", "foreign amax", be.split(x, bits), S.split(x, bits))
    rows = 8192 * 256 + 3
    big = R.f32(rs.randn(rows, 8))
    big[rows - 1, 7] = 300.0
    bits = S.amax_bits(big)
    LEDGER.exact("split planes, float4", "grid stride", be.split(big, bits), S.split(big, bits))


def test_split_planes_special(be):
    row_split_planes_special(be)


BN_SPLIT_CASES = [(kind, n, pitched) for kind in G.KINDS for n in (4, 12, 1500) for pitched in (False, True)]


def row_bn_apply_split(be, kind, n, pitched):
    """xv_bn_apply_split without an activation, with ReLU, with a prelu vector and with a constant slope; n = 4 (half a chunk), 12 (n % 8 = 4: a
    chunk whose second quad is beyond n), 1500; ldz > n.  The planes bit for bit against the model applied to the float32 value of the fused
    z scale + shift (S.bn_apply_value); amax is the exact maximum of those values, as bn_finalize's output range supplies it."""
    rs = np.random.RandomState(seed_of("bn apply split", kind, n, pitched))
    rows = 37
    z = R.make_z(rs, rows, n)
    gamma, beta = R.make_affine(rs, n, negative=1)
    scale, shift = R.f32(gamma / np.sqrt(4.0 + 1e-3)), R.f32(beta - 0.3 * gamma)
    relu, slope, _ = slope_of(rs, kind, n)
    y = S.bn_apply_value(z, scale, shift, relu, slope)
    bits = S.amax_bits(y)
    got = be.bn_apply_split(z, scale, shift, relu, slope, bits, n + 4 if pitched else None)
    LEDGER.exact("bn apply split, %s" % kind, "planes%s" % (" (ldz > n)" if pitched else ""), got, S.split(y, bits))


@pytest.mark.parametrize("kind,n,pitched", BN_SPLIT_CASES)
def test_bn_apply_split(be, kind, n, pitched):
    row_bn_apply_split(be, kind, n, pitched)


# =========================================================================================== NT rows
def _nt(name, segs, t, c, k, o, **opts):
    return dict(name=name, segs=segs, t=t, c=c, k=k, o=o, **opts)


def boundary_rows(bm):
    """Per k the last a_rps that takes the context-window kernel with bm-row tiles and the first that does not (P.CONV_BOUNDARY), with enough
    segments for two whole tiles and a ragged third; at the boundary the channels give 1, 2 and 3 chunks; N walks over 8, 96, 128, 136.
    kernel: what a process without XV_CONV_WR runs; bm4: the tile height under XV_CONV_WR=4 (a row the 256-row rule turns away takes 128-row
    tiles, and every row at a boundary of the 128-row rule lies outside the 256-row one)."""
    rows = []
    widths = (8, 96, 128, 136)
    for i, (k, (inside, outside)) in enumerate(sorted(P.CONV_BOUNDARY[bm].items())):
        for j, (rps, c) in enumerate(((inside, 25 + 2 * i), (inside, 64), (inside, 96), (outside, 32 - i))):
            segs = (2 * bm + 4) // rps + 1
            kernel = P.CONV if (bm == 256 or rps == inside) else P.GENERIC
            rows.append(_nt("k%d-rps%d-c%d" % (k, rps, c), segs, rps, c, k, widths[(i + j) % 4], kernel=kernel,
                            bm4=256 if (bm == 256 and rps == inside) else 128))
    return rows


# forward: t = t_out (the rows of a segment); data gradient: t = t_out + k - 1 (its rows of a segment), c = the width of dz, o = the width of dx
FORWARD_ROWS = boundary_rows(128) + [
    _nt("k5-c30-ldz", 5, 36, 30, 5, 136, kernel=P.CONV, bm4=128, ldz=140),                                            # ldc > N
    _nt("k3-c64-nobias", 3, 50, 64, 3, 96, kernel=P.CONV, bm4=256, bias=False),
    _nt("k5-c32-zero", 3, 40, 32, 5, 8, kernel=P.CONV, bm4=256, zero=True),
    # the generic kernel: K % 32 in {8, 16, 24, 0}, 1 ... 4 K-steps, one-row segments, lda % 32 != 0 with taps, M around a tile
    _nt("g-c5-k1", 1, 127, 5, 1, 96, kernel=P.GENERIC, steps=(1, 8)), _nt("g-c13-k1", 1, 128, 13, 1, 8, kernel=P.GENERIC, steps=(1, 16)),
    _nt("g-c24-k1", 1, 129, 24, 1, 136, kernel=P.GENERIC, steps=(1, 24)), _nt("g-c37-k1", 1, 1, 37, 1, 128, kernel=P.GENERIC, steps=(2, 8)),
    _nt("g-c8-k3", 4, 40, 8, 3, 96, kernel=P.GENERIC, steps=(1, 24)), _nt("g-c16-k3", 140, 1, 16, 3, 136, kernel=P.GENERIC, steps=(2, 16)),
    _nt("g-c24-k3", 3, 43, 24, 3, 8, kernel=P.GENERIC, steps=(3, 8), ldz=12), _nt("g-c40-k3", 2, 70, 40, 3, 128, kernel=P.GENERIC, steps=(4, 24)),
    _nt("g-c32-k1", 2, 70, 32, 1, 96, kernel=P.GENERIC, steps=(1, 32)), _nt("g-c64-k1", 2, 64, 64, 1, 136, kernel=P.GENERIC, steps=(2, 32), bias=False),
    _nt("g-c96-k1", 1, 130, 96, 1, 8, kernel=P.GENERIC, steps=(3, 32)), _nt("g-c16-k1-zero", 1, 20, 16, 1, 96, kernel=P.GENERIC, zero=True),
]
DGRAD_ROWS = [dict(r, name="d-" + r["name"]) for r in boundary_rows(128)] + [
    _nt("d-g-c40-k3", 3, 45, 40, 3, 136, kernel=P.GENERIC, steps=(4, 24)), _nt("d-g-c16-k1", 1, 129, 16, 1, 96, kernel=P.GENERIC, steps=(1, 16)),
    _nt("d-k5-c64-zero", 3, 40, 64, 5, 8, kernel=P.CONV, bm4=256, zero=True),
]
# the 256-row tiles: their own boundary pairs and the conv rows above (bm4: which of them the 256-row rule admits)
FORWARD_ROWS_256 = boundary_rows(256) + [r for r in FORWARD_ROWS if r["kernel"] == P.CONV]
DGRAD_ROWS_256 = [dict(r, name="d-" + r["name"]) for r in boundary_rows(256)] + [r for r in DGRAD_ROWS if r["kernel"] == P.CONV]


def nt_problem(role, row):
    if role == "fwd":
        return P.forward_problem(row["segs"], row["t"] + row["k"] - 1, P.align8(row["c"]), row["k"], row["o"])
    return P.dgrad_problem(row["segs"], row["t"] - row["k"] + 1, P.align8(row["c"]), row["k"], row["o"])


def asserted_form(role, row, stats=False, bwd=False):
    """The row's form through the restatement and the hook: the kernel and the tile height the row was written for (and the K-steps and the
    valid halfs of the last one, where the row names them)."""
    form = P.both_nt(*nt_problem(role, row), stats=stats, bwd=bwd, conv_wr=CONV_WR)
    kernel = P.GENERIC if bwd else row["kernel"]
    bm = row["bm4"] if (CONV_WR == 4 and kernel == P.CONV) else 128
    assert form[:2] == (kernel, bm), "%s %s: written for kernel %d with %d-row tiles, the library runs %r" % (role, row["name"], kernel, bm, form)
    if "steps" in row:
        assert form[6:8] == row["steps"], (row["name"], form)
    return form


def nt_operands(role, row, family):
    """x [segs][t_in][c] and kern [k][c][o] for a forward row, dz [segs][t_out][c] and kern [k][o][c] for a data-gradient row (there c is dz's
    width and o dx's), bias; family: random | a-wide | b-wide (position-coded integers, the wide operand carrying both pieces)."""
    segs, t, c, k, o = (row[key] for key in ("segs", "t", "c", "k", "o"))
    t_a = t + k - 1 if role == "fwd" else t - k + 1
    kshape = (k, c, o) if role == "fwd" else (k, o, c)
    if family == "random":
        rs = np.random.RandomState(seed_of("nt", role, row["name"]))
        if role == "fwd":
            a, kern, bias, _ = S.make_operands(rs, segs, t_a, c, k, o)
        else:
            _, kern, bias, a = S.make_operands(rs, segs, t, o, k, c)
    else:
        terms = k * c
        a = S.coded_wide((segs, t_a, c), terms, 1) if family == "a-wide" else S.coded_small((segs, t_a, c), 1)
        kern = S.coded_small(kshape, 2) if family == "a-wide" else S.coded_wide(kshape, terms, 2)
        bias = S.coded_small((o,), 3)
    if row.get("zero"):
        a = np.zeros_like(a)
    return a, kern, (bias if row.get("bias", True) and role == "fwd" else None)


def check_tile_stats(form_name, got, kernel):
    ref, b = S.tile_stats(got["z"], kernel)
    LEDGER.check(form_name, "tile sums", got["part"][0], ref[0], b[0])
    LEDGER.check(form_name, "tile centred squares", got["part"][1], ref[1], b[1])
    LEDGER.exact(form_name, "tile min", got["part"][2], R.f32(ref[2]))
    LEDGER.exact(form_name, "tile max", got["part"][3], R.f32(ref[3]))


def row_nt_forward(be, row):
    """xv_affine_forward_f16x3, plain and with the statistics epilogue: z bit for bit on the coded operands, within S.forward_bound on the random
    ones; the statistics against R.col_stats on the z the launch returned (min and max exact); a zero operand gives z = bias exactly."""
    for stats in (False, True):
        form = asserted_form("fwd", row, stats=stats)
        name = P.nt_form_name(form, stats=stats)
        for family in ("a-wide", "b-wide", "random"):
            x, kern, bias = nt_operands("fwd", row, family)
            got = be.forward(x, kern, bias, stats, row.get("ldz"), CONV_WR)
            if family == "random" and not row.get("zero"):
                ref, bound = S.forward_bound(x, kern, bias, got["ax"], got["aw"], form)
                LEDGER.check(name, "z", got["z"], ref, bound)
            else:
                LEDGER.exact(name, "z (%s)" % ("zero operand" if row.get("zero") else "coded"), R.f64(got["z"]), S.forward(x, kern, bias))
            if stats:
                check_tile_stats(name, got, form[0])


def row_nt_dgrad(be, row):
    """xv_affine_dgrad_f16x3 on dz planes padded by k - 1 frames (the halo rows of a segment read the zero frames of its neighbours' pads)."""
    form = asserted_form("dgrad", row)
    name = P.nt_form_name(form)
    assert row["t"] >= row["k"], "a data-gradient row needs t_out = t - k + 1 >= 1"
    for family in ("a-wide", "b-wide", "random"):
        dz, kern, _ = nt_operands("dgrad", row, family)
        got = be.dgrad(dz, kern, None, CONV_WR)
        if family == "random" and not row.get("zero"):
            ref, bound = S.dgrad_bound(dz, kern, row["t"], got["adz"], got["aw"], form)
            LEDGER.check(name, "dx", got["dx"], ref, bound)
        else:
            LEDGER.exact(name, "dx (%s)" % ("zero operand" if row.get("zero") else "coded"), R.f64(got["dx"]), S.dgrad(dz, kern, row["t"]))


@pytest.mark.parametrize("row", FORWARD_ROWS, ids=[r["name"] for r in FORWARD_ROWS])
def test_nt_forward(be, row):
    row_nt_forward(be, row)


@pytest.mark.parametrize("row", DGRAD_ROWS, ids=[r["name"] for r in DGRAD_ROWS])
def test_nt_dgrad(be, row):
    row_nt_dgrad(be, row)


# segs, t_out, k, width of dz (o), width of dx (c): the two shapes of tests/test_gpu_ops_f16x3.py, a ragged last row tile with N % 128 != 0, one row tile
BWD_EPI_ROWS = [(5, 57, 5, 512, 512), (3, 300, 1, 512, 512), (3, 50, 3, 40, 136), (1, 20, 5, 64, 8)]


def row_nt_bwd_epilogue(be, segs, t_out, k, o, c):
    """xv_affine_dgrad_bnstats_f16x3 (EPI 2, always the generic kernel): dx within the data gradient's bound and - the same products in the same
    order - bit-equal to the plain launch where that takes the generic kernel too; the partials against S.bwd_partials on the dx the launch
    returned, mask-ambiguous elements added to the bounds, max |dd| exact where a tile's column has none."""
    prob = P.dgrad_problem(segs, t_out, P.align8(o), k, c)
    form = P.both_nt(*prob, bwd=True, conv_wr=CONV_WR)
    assert form[0] == P.GENERIC
    name = P.nt_form_name(form, bwd=True)
    rs = np.random.RandomState(seed_of("bwd epilogue", segs, t_out, k, o, c))
    _, kern, _, dz = S.make_operands(rs, segs, t_out + k - 1, c, k, o)      # kern [k][c][o]
    rows = segs * (t_out + k - 1)
    z = R.make_z(rs, rows, c)
    gamma, beta = R.make_affine(rs, c, negative=1)
    mean, var = R.f32(z.mean(axis=0)), z.var(axis=0)
    invstd = R.f32(1 / np.sqrt(var + 1e-3))
    scale = R.f32(R.f64(gamma) * R.f64(invstd))
    shift = R.f32(R.f64(beta) - R.f64(mean) * R.f64(scale))
    bwd = dict(z=z, scale=scale, shift=shift, mean=mean, invstd=invstd)
    got = be.dgrad(dz, kern, bwd, CONV_WR)
    ref, bound = S.dgrad_bound(dz, kern, t_out + k - 1, got["adz"], got["aw"], form)
    LEDGER.check(name, "dx", got["dx"], ref, bound)
    if P.nt_form(*prob, conv_wr=CONV_WR)[0] == P.GENERIC:
        LEDGER.exact(name, "dx against the plain launch", got["dx"], be.dgrad(dz, kern, None, CONV_WR)["dx"])
    pref, pb, amb, keep = S.bwd_partials_bound(got["dx"], z, scale, shift, mean, invstd)
    LEDGER.check(name, "sum dd", got["part"][:, 0], pref[:, 0], pb[:, 0])
    LEDGER.check(name, "sum dd xhat", got["part"][:, 1], pref[:, 1], pb[:, 1])
    LEDGER.check(name, "max |dd|", got["part"][:, 2], pref[:, 2], np.zeros_like(pref[:, 2]), keep)
    note_share(name, "bwd epilogue %r" % ((segs, t_out, k, o, c),), amb)


@pytest.mark.parametrize("segs,t_out,k,o,c", BWD_EPI_ROWS)
def test_nt_bwd_epilogue(be, segs, t_out, k, o, c):
    row_nt_bwd_epilogue(be, segs, t_out, k, o, c)


def test_forward_ldz_through_ops(be):
    """tf_kaldi_speaker_amd.ops.affine_forward_f16x3(ldz=): the same launch into a pitched result."""
    row = FORWARD_ROWS[0]
    x, kern, bias = nt_operands("fwd", row, "random")
    ops, t = be.ops, be.torch
    xp = ops.split_planes(be.dev(x.reshape(-1, row["c"])))
    wtp = ops.split_planes(be.dev(S.weights_fwd(kern, xp.ld)))
    d_bias = be.dev(bias)
    z0 = ops.affine_forward_f16x3(xp, row["segs"], row["t"] + row["k"] - 1, row["k"], wtp, d_bias, row["o"])
    z1 = ops.affine_forward_f16x3(xp, row["segs"], row["t"] + row["k"] - 1, row["k"], wtp, d_bias, row["o"], ldz=row["o"] + 4)
    assert z1.shape == z0.shape and z1.stride(0) == row["o"] + 4 and t.equal(z0, z1.contiguous())


# =========================================================================================== TN rows
def _tn(name, segs, t_out, c, k, o, pad=None, l2=0.0, **want):
    return dict(name=name, segs=segs, t=t_out, c=c, k=k, o=o, pad=pad, l2=l2, **want)


# rps = t_out; M = k * ceil8(c) in {8 ... 2560}, N = ceil8(o) in {8, 104, 136, 512}: c < c_ld and o < o_ld, ragged M and N tiles
TN_ROWS = [
    _tn("rps1", 3000, 1, 8, 3, 4, form="tn all-ragged, ragged last stage, splits", splits=47),                 # the float division up to r = 2999
    _tn("rps3", 1000, 3, 12, 2, 100, l2=1e-2, form="tn all-ragged, ragged last stage, splits"),
    _tn("rps7", 448, 7, 30, 3, 132, form="tn all-ragged, whole last stage, splits", splits=49),                # R % 32 = 0
    _tn("rps31", 100, 31, 30, 5, 132, l2=1e-2, form="tn all-ragged, ragged last stage, splits", splits=33),    # M = 160, N = 136: both tiles ragged
    _tn("rps7-r63", 9, 7, 30, 1, 100, pad=2, form="tn all-ragged, ragged last stage, 1 split"),                # R % 32 = 31
    _tn("rps16-r64", 4, 16, 30, 2, 4, pad=0, form="tn all-ragged, whole last stage, 1 split"),                 # unpadded dz: x's pitch alone keeps the segments
    _tn("rps20-r20", 1, 20, 30, 5, 132, form="tn all-ragged, ragged last stage, 1 split"),                     # R < 32
    _tn("rps32", 20, 32, 30, 5, 132, l2=1e-2, form="tn steady, whole last stage, splits", splits=10),          # a wrap every stage
    _tn("rps33", 20, 33, 30, 3, 100, form="tn steady, ragged last stage, splits", splits=7, mid_segment=True),
    _tn("rps57", 5, 57, 30, 5, 132, pad=0, form="tn steady, ragged last stage, splits", splits=3),
    _tn("rps33-r33", 1, 33, 30, 5, 100, l2=1e-2, form="tn steady, ragged last stage, 1 split"),                # R % 32 = 1
    _tn("rps32-r64", 2, 32, 30, 1, 132, pad=1, form="tn steady, whole last stage, 1 split"),
    _tn("rps80-r160", 2, 80, 30, 5, 4, form="tn steady, whole last stage, splits", splits=2),
    _tn("rps64-cap", 8, 64, 508, 5, 512, l2=1e-2, form="tn steady, whole last stage, splits", splits=6),       # M = 2560, N = 512: 80 tiles, 512 / 80 = 6
    # r / rps by a float product first misses at r = 10 186 169 (rps = 15; P.tn_division_misses): the one size at which the +-1 correction of the
    # per-row stages can act.  dz is zero outside a window of 64 rows around it, so that the sums stay exact; one coded run alone
    _tn("rps15-r10M", 679081, 15, 1, 2, 4, form="tn all-ragged, ragged last stage, splits", splits=512, window=(10186169 - 32, 10186169 + 32)),
    _tn("dense-r20", 1, 20, 30, 1, 100, form="tn collapsed, ragged last stage, 1 split"),
    _tn("dense-r64", 2, 32, 30, 1, 132, l2=1e-2, form="tn collapsed, whole last stage, 1 split"),
    _tn("dense-r65", 5, 13, 30, 1, 4, form="tn collapsed, ragged last stage, 1 split"),
    _tn("dense-r256", 4, 64, 30, 1, 100, form="tn collapsed, whole last stage, splits", splits=4),
    _tn("dense-r300", 3, 100, 30, 1, 132, form="tn collapsed, ragged last stage, splits", splits=5, twin_pad=1),
]


def tn_problem(row, pad=None):
    k = row["k"]
    pad = (k - 1 if row["pad"] is None else row["pad"]) if pad is None else pad
    return (k * P.align8(row["c"]), P.align8(row["o"]), row["segs"] * row["t"], row["t"], row["t"] + k - 1, row["t"] + 2 * pad), pad


def tn_operands(row, family):
    segs, t_out, c, k, o = (row[key] for key in ("segs", "t", "c", "k", "o"))
    if family == "random":
        x, kern, _, dz = S.make_operands(np.random.RandomState(seed_of("tn", row["name"])), segs, t_out + k - 1, c, k, o)
        return x, dz, kern, row["l2"]
    terms = segs * t_out
    if "window" in row:      # dz [rows lo ... hi) coded, zero elsewhere
        lo, hi = row["window"]
        dz = np.zeros((segs * t_out, o), np.float32)
        dz[lo:hi] = S.coded_wide((hi - lo, o), hi - lo, 5)
        return S.coded_small((segs, t_out + k - 1, c), 4), dz.reshape(segs, t_out, o), S.coded_small((k, c, o), 6), 0.0
    x = S.coded_wide((segs, t_out + k - 1, c), terms, 4) if family == "a-wide" else S.coded_small((segs, t_out + k - 1, c), 4)
    dz = S.coded_small((segs, t_out, o), 5) if family == "a-wide" else S.coded_wide((segs, t_out, o), terms, 5)
    return x, dz, S.coded_small((k, c, o), 6), 2.0 if row["l2"] else 0.0


def row_tn(be, row):
    """xv_affine_wgrad_f16x3 with dz planes padded as the engine passes them (dz_seg_pitch = t_out + 2 pad, dz_row0 = pad; pad = k - 1 unless the
    row says otherwise): bit for bit on the coded operands, within S.wgrad_bound on the random ones; l2_scale zero and non-zero."""
    prob, pad = tn_problem(row)
    plan = P.both_tn(*prob)
    assert P.tn_form(*prob) == row["form"], (row["name"], P.tn_form(*prob), plan)
    if "splits" in row:
        assert plan[1] == row["splits"], (row["name"], plan)
    if row.get("mid_segment"):
        assert P.tn_stages(*prob)["mid_segment"]
    if "window" in row:
        assert P.tn_division_misses(row["t"], *row["window"]).size > 0 and row["window"][1] <= prob[2]
    for family in ("b-wide",) if "window" in row else ("a-wide", "b-wide", "random"):
        x, dz, kern, l2 = tn_operands(row, family)
        got = be.wgrad(x, dz, kern, l2, pad)
        if family == "random":
            ref, bound = S.wgrad_bound(x, dz, kern, l2, got["ax"], got["adz"], plan)
            LEDGER.check(row["form"], "dkernel", got["dk"], ref, bound)
            if "twin_pad" in row:      # the same numbers behind a padded dz: not collapsed, the steady stages
                prob2, pad2 = tn_problem(row, row["twin_pad"])
                plan2 = P.both_tn(*prob2)
                assert plan2[3] == 0 and plan[3] == 1 and plan2[1:3] == plan[1:3]
                twin = be.wgrad(x, dz, kern, l2, pad2)
                ref2, bound2 = S.wgrad_bound(x, dz, kern, l2, twin["ax"], twin["adz"], plan2)
                LEDGER.check(P.tn_form(*prob2), "dkernel", twin["dk"], ref2, bound2)
                LEDGER.check("tn collapsed against padded", "dkernel", got["dk"], twin["dk"], bound + bound2)
        else:
            LEDGER.exact(row["form"], "dkernel (coded)", R.f64(got["dk"]), S.wgrad(x, dz, kern, l2))


@pytest.mark.parametrize("row", TN_ROWS, ids=[r["name"] for r in TN_ROWS])
def test_tn(be, row):
    row_tn(be, row)


def forms_of_rows(conv_wr=0):
    """The forms the rows above assert (from the restatement alone: nothing runs)."""
    fwd, dg = (FORWARD_ROWS_256, DGRAD_ROWS_256) if conv_wr == 4 else (FORWARD_ROWS, DGRAD_ROWS)
    seen = set()
    for row in fwd:
        for stats in (False, True):
            seen.add(P.nt_form_name(P.nt_form(*nt_problem("fwd", row), stats=stats, conv_wr=conv_wr), stats=stats))
    for row in dg:
        seen.add(P.nt_form_name(P.nt_form(*nt_problem("dgrad", row), conv_wr=conv_wr)))
    if conv_wr == 0:
        for segs, t_out, k, o, c in BWD_EPI_ROWS:
            seen.add(P.nt_form_name(P.nt_form(*P.dgrad_problem(segs, t_out, P.align8(o), k, c), bwd=True), bwd=True))
        for row in TN_ROWS:
            seen.add(P.tn_form(*tn_problem(row)[0]))
    return seen


def test_rows_cover_every_form():
    assert forms_of_rows(0) == P.nt_forms(0) | P.tn_forms()
    assert forms_of_rows(4) >= {f for f in P.nt_forms(4) if "conv 256" in f}


# =========================================================================================== refusals
def test_refusals(be):
    """Each by the name of its message, before anything is launched (the results stay NaN).  "gemm16_tn: splits must come from xv_tn16_splits"
    guards the launcher against its callers inside the library: xv_affine_wgrad_f16x3 always plans with xv_tn16_splits, so no argument
    of the C interface reaches it; what it checks (cdiv(R, r_chunk) == splits) is asserted of every plan in tests/test_gemm16_plans.py."""
    from tf_kaldi_speaker_amd import _lib as L
    t, p = be.torch, be.ops._p
    x = be.dev(np.ones((40, 12), np.float32))
    xp = be.ops.split_planes(x)                       # ld = 16
    wtp = be.ops.split_planes(be.dev(np.ones((8, 16), np.float32)))
    z = t.full((40 * 8,), float("nan"), dtype=t.float32, device=be.dev_name)

    def forward(data, c_ld, stride=None):
        return L.call("xv_affine_forward_f16x3", be.stream(), data, C.c_size_t(xp.stride if stride is None else stride), p(xp.amax), 1, 40, c_ld, 1,
                      p(wtp.data), C.c_size_t(wtp.stride), p(wtp.amax), None, p(z), 8, 8, None)

    with pytest.raises(L.XvError, match="lda/ldb must be multiples of 8"):
        forward(p(xp.data), 12)
    with pytest.raises(L.XvError, match="planes must be 16-byte aligned"):
        forward(C.c_void_p(xp.data.data_ptr() + 2), 16)
    with pytest.raises(L.XvError, match="planes must be 16-byte aligned"):
        forward(p(xp.data), 16, xp.stride + 4)
    with pytest.raises(L.XvError, match="a plane spans 4 GB"):      # extents only: 2^21 segments of 64 frames of 16 halfs
        L.call("xv_affine_forward_f16x3", be.stream(), p(xp.data), C.c_size_t(xp.stride), p(xp.amax), 1 << 21, 64, 16, 1, p(wtp.data),
               C.c_size_t(wtp.stride), p(wtp.amax), None, p(z), 8, 8, None)
    assert bool(t.isnan(z).all())
    with pytest.raises(L.XvError, match="n and ldz must be multiples of 4"):
        L.call("xv_bn_apply_split", be.stream(), p(x), 40, 6, 12, p(x), p(x), 1, p(xp.amax), p(xp.data), 8, C.c_size_t(40 * 8))
    row = TN_ROWS[8]
    xs, dz, kern, l2 = tn_operands(row, "random")
    with pytest.raises(L.XvError, match="workspace too small"):
        be.wgrad(xs, dz, kern, l2, None, ws_short=1)


# =========================================================================================== the 256-row tiles
if CONV_WR == 4:
    @pytest.mark.parametrize("row", FORWARD_ROWS_256, ids=["wr4-" + r["name"] for r in FORWARD_ROWS_256])
    def test_nt_forward_256(be, row):
        row_nt_forward(be, row)

    @pytest.mark.parametrize("row", DGRAD_ROWS_256, ids=["wr4-" + r["name"] for r in DGRAD_ROWS_256])
    def test_nt_dgrad_256(be, row):
        row_nt_dgrad(be, row)


def test_context_window_rows_with_256_row_tiles():
    """XV_CONV_WR is read once per process: the rows of the 256-row tiles (the conv rows above and the two boundary pairs of their own) run
    in one fresh child, selected by their parameter ids."""
    assert CONV_WR == 0, "the child must not start children"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", os.path.abspath(__file__), "-k", "wr4-"],
                       cwd=root, env=dict(os.environ, XV_CONV_WR="4"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
