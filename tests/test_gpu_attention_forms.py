"""Every kernel form of csrc/xv_attention.hip at the smallest shapes at which it can still go wrong, each output against a float64 evaluation
of the same operation on the same float32 inputs (tests/attention_ref.py) within a bound derived from the kernel's own order of operations
- per element, never relative to the tensor's largest entry.  A score row first asserts its form (vector / scalar) through the
restatement of tests/test_segment_plans.py and the library's hook, so a row that silently moves to the other kernel fails.

The rows are functions of a backend: the tests here hand them the GPU (class GpuOps, the C entry points called through _lib.call on
NaN-surrounded buffers), tests/test_attention_ref.py hands the same rows a plain float32 NumPy evaluation first.  $XV_BOUNDS_OUT names a
file that receives the largest ratio to its bound per form and the wall time of the module.

Branches named here that no earlier op-level row reaches: att_score_kernel<false> (n % 4 != 0, a pitch % 4 != 0, a base off 16 bytes), the
second pass of att_score_kernel<true> and att_pool_dw_kernel beyond 2 048 columns, act = 1 in the score and the key backward, the stride
loop / an empty wave / large offsets / a dominant frame in the softmax kernels, the four sides of sd <= 1e-6 and scale == NULL, relu = 0
and the slope form in att_pool_dw_kernel, fewer rows than row lanes / a row count on the 64-row chunk / dbias == NULL in att_key_bwd_kernel,
and a second trip of the grid-stride loops of key_activation_kernel and add_inplace_kernel."""
import ctypes as C
import time

import numpy as np
import pytest

import attention_ref as A
import bn_pool_ref as R
import test_gpu_bn_pool_forms as G
import test_segment_plans as P
from test_gpu_bn_pool_forms import seed_of, slope_of

pytestmark = pytest.mark.gpu

LEDGER = R.Ledger()
SHARES = {}
GRID_TRIP = 8192 * 256         # elements (key_activation) or float4s (add_inplace) one trip of the grid-stride loop covers


def note_share(form, row, amb):
    share = float(np.mean(amb)) if amb.size else 0.0
    SHARES[form] = max(SHARES.get(form, 0.0), share)
    assert share <= R.MAX_AMBIGUOUS_SHARE, "%s: %.3g of the elements are mask-ambiguous (cap %.0e): change the seed" % (row, share, R.MAX_AMBIGUOUS_SHARE)


def write_ledger(tag, seconds):
    G.write_ledger(tag, seconds, LEDGER, SHARES, "attention forms")
    LEDGER.worst.clear()      # (also without $XV_BOUNDS_OUT: the CPU module of these rows shares this ledger)
    SHARES.clear()


class GpuOps(G.GpuOps):
    """float32 NumPy in, float32 NumPy out; every device buffer is surrounded by NaN, which must still be there afterwards."""

    def __init__(self):
        super(GpuOps, self).__init__()
        from tf_kaldi_speaker_amd import _lib
        self.lib = _lib

    def out(self, count):
        """A result buffer of count floats with 4 NaN floats behind it."""
        buf = self.torch.full((count + 4,), float("nan"), dtype=self.torch.float32, device=self.dev_name)
        return buf, buf[:count]

    def done(self, buf, count, what):
        h = self.host(buf)
        assert np.all(np.isnan(h[count:])), "%s wrote beyond its result" % what
        return h[:count].copy()

    def vec(self, a):
        return None if a is None else self.view(np.reshape(a, (1, -1)))[0]

    def stream(self):
        return C.c_void_p(self.torch.cuda.current_stream().cuda_stream)

    def att_score(self, zk, act, q, scale, ldz=None, offset=0, want_form=None):
        rows, n = zk.shape
        v, dq = self.view(zk, ldz, offset), self.vec(q)
        if want_form is not None:
            got = P.lib_att_score_form(n, v.stride(0), v.data_ptr(), dq.data_ptr())
            assert got == want_form == P.att_score_form(n, v.stride(0), v.data_ptr(), dq.data_ptr()), (got, want_form)
        buf, score = self.out(rows)
        self.lib.call("xv_att_score", self.stream(), self.ops._p(v), rows, n, v.stride(0), int(act), self.ops._p(dq), float(scale), self.ops._p(score))
        return self.done(buf, rows, "xv_att_score")

    def softmax(self, score):
        b, t = score.shape
        buf, w = self.out(b * t)
        d_score = self.vec(score)      # (every device tensor stays in a local until the result is back: a temporary's memory is reused by the next allocation)
        self.lib.call("xv_softmax_segments", self.stream(), self.ops._p(d_score), b, t, self.ops._p(w))
        return self.done(buf, b * t, "xv_softmax_segments").reshape(b, t)

    def softmax_backward(self, w, dw):
        b, t = w.shape
        buf, ds = self.out(b * t)
        d_w, d_dw = self.vec(w), self.vec(dw)
        self.lib.call("xv_softmax_segments_backward", self.stream(), self.ops._p(d_w), self.ops._p(d_dw), b, t, self.ops._p(ds))
        return self.done(buf, b * t, "xv_softmax_segments_backward").reshape(b, t)

    def att_pool_dw(self, z, b, t, scale, shift, relu, slope, pool, dpool):
        n = z.shape[1]
        buf, dw = self.out(b * t)
        d_z, d_scale, d_shift, d_pool, d_dpool = self.view(z), self.vec(scale), self.vec(shift), self.view(pool), self.view(dpool)
        with self.activation(slope):
            self.lib.call("xv_att_pool_backward_weights", self.stream(), self.ops._p(d_z), b, t, n, self.ops._p(d_scale),
                          self.ops._p(d_shift), int(relu), self.ops._p(d_pool), self.ops._p(d_dpool), self.ops._p(dw))
        return self.done(buf, b * t, "xv_att_pool_backward_weights").reshape(b, t)

    def key_backward(self, zk, act, q, scale, ds, want_dbias=True):
        rows, n = zk.shape
        b1, dzk = self.out(rows * n)
        b2, dq = self.out(n)
        b3, db = self.out(n)
        wp, wb = self.ops._ws(dzk)
        d_zk, d_q, d_ds = self.view(zk), self.vec(q), self.vec(ds)
        self.lib.call("xv_att_key_backward", self.stream(), self.ops._p(d_zk), rows, n, int(act), self.ops._p(d_q), float(scale),
                      self.ops._p(d_ds), self.ops._p(dzk), self.ops._p(dq), self.ops._p(db if want_dbias else None), wp, wb)
        db_h = self.done(b3, n, "xv_att_key_backward (dbias)") if want_dbias else None
        if not want_dbias:
            assert np.all(np.isnan(self.host(b3))), "xv_att_key_backward wrote a bias gradient nobody asked for"
        return self.done(b1, rows * n, "xv_att_key_backward (dzk)").reshape(rows, n), self.done(b2, n, "xv_att_key_backward (dquery)"), db_h

    def key_activation(self, z, act):
        count = z.size
        buf, y = self.out(count)
        d_z = self.vec(z)
        self.lib.call("xv_key_activation", self.stream(), self.ops._p(d_z), C.c_size_t(count), int(act), self.ops._p(y))
        return self.done(buf, count, "xv_key_activation").reshape(z.shape)

    def add_inplace(self, y, x=None):
        count = y.size
        buf, dy = self.out(count)
        dy.copy_(self.dev(y))
        dx = dy if x is None else self.vec(x)
        self.lib.call("xv_add_inplace", self.stream(), self.ops._p(dy), self.ops._p(dx), C.c_size_t(count))
        return self.done(buf, count, "xv_add_inplace")


@pytest.fixture(scope="module")
def be():
    t0 = time.time()
    yield GpuOps()
    write_ledger("gpu", time.time() - t0)


# =========================================================================================== score
SCORE_VECTOR = [(n, pad) for n in (4, 252, 256, 260, 1500, 2048, 2052) for pad in (0, 4)]
SCORE_SCALAR = [(1, 1, 0), (63, 63, 0), (65, 65, 0), (65, 68, 0), (1499, 1499, 0), (1499, 1500, 0), (256, 257, 0), (256, 256, 1)]      # n, pitch, base offset in floats
SCORE_CASES = [(act, fam) for act in (0, 1, 3) for fam in ("base", "hetero")]


def row_att_score(be, act, family):
    """xv_att_score.  Vector form (att_score_kernel<true>): n in {4, 252, 256, 260} around one quad per lane (64 lanes x 4 columns), 1 500,
    2 048 = the last width of one pass and 2 052 = the first of a second pass; a pitch of n and of n + 4 with NaN in the pad.  Scalar form
    (att_score_kernel<false>): n in {1, 63, 65, 1 499}, a pitch that is no multiple of 4, n = 256 at a pitch of 257 and n = 256 with the base
    one float off a 16-byte boundary.  rows in {1, 3, 5}: a block's four waves with 1, 3 and 4 + 1 valid rows.  scale 1 and 1 / sqrt(n).
    act = 1 runs on exact zeros in zk, and row 0 is then all zeros and negatives: its score is exactly 0.
    L = ceil(n / 256) + 2 + 6 (vector), ceil(n / 64) + 6 (scalar): A.score_chain.  Both forms on the same data agree within the sum of their bounds."""
    rs = np.random.RandomState(seed_of("att_score", act, family))
    cases = [(n, n + pad, 0, P.VECTOR) for n, pad in SCORE_VECTOR] + [(n, ld, off, P.SCALAR) for n, ld, off in SCORE_SCALAR]
    for n, ldz, offset, form in cases:
        assert P.att_score_form(n, ldz, P.BASE + 4 * offset, P.BASE) == form
        passes = R.cdiv(R.cdiv(n, 4), 64 * 8)
        assert passes == (2 if n > A.SCORE_PASS else 1)
        for rows in (1, 3, 5):
            for scale in (1.0, 1.0 / np.sqrt(n)):
                zk, q = A.make_key(rs, rows, n, family, zeros=act == 1)
                if act == 1:
                    zk[0] = -np.abs(zk[0])
                got = be.att_score(zk, act, q, scale, ldz, offset, form)
                ref, bound = A.att_score(zk, act, q, scale), A.att_score_bound(zk, act, q, scale, form == P.VECTOR)
                if n == 1500 and family == "base":      # test_self_attention_pieces of tests/test_gpu_ops.py: 2e-5 of the largest entry
                    bound = LEDGER.capped(bound, ref, 2e-5) if rows == 5 else bound
                name = "att_score %s%s" % ("vector" if form == P.VECTOR else "scalar", ", second pass" if form == P.VECTOR and passes == 2 else "")
                LEDGER.check(name, "act %d" % act, got, ref, bound)
                if act == 1:
                    LEDGER.exact(name, "a row without a positive key", got[0], np.float32(0))
                if form == P.VECTOR and n in (256, 2052) and scale == 1.0:      # the scalar kernel on the same data
                    other = be.att_score(zk, act, q, scale, n, 1, P.SCALAR)
                    LEDGER.check("att_score vector against scalar", "act %d" % act, got, other,
                                 bound + A.att_score_bound(zk, act, q, scale, False))


@pytest.mark.parametrize("act,family", SCORE_CASES)
def test_att_score(be, act, family):
    row_att_score(be, act, family)


# =========================================================================================== softmax over frames
SOFTMAX_T = (1, 2, 63, 64, 65, 255, 256, 257, 600)
SOFTMAX_FAMILIES = ("randn", "offset", "dominant", "equal")
SOFTMAX_CASES = [(t, fam) for t in SOFTMAX_T for fam in SOFTMAX_FAMILIES]


def softmax_scores(rs, b, t, family):
    if family == "equal":
        return np.full((b, t), 0.37, np.float32)
    s = rs.randn(b, t)
    if family == "offset":
        s = s + 1e4
    if family == "dominant":
        s[np.arange(b), rs.randint(0, t, b)] += 120.0
    return R.f32(s)


def row_softmax(be, t, family):
    """softmax_segments_kernel and softmax_segments_bwd_kernel, b = 3 chunks, t in {1, 2, 63, 64, 65} (one wave, three waves without an element),
    {255, 256, 257} around the 256 threads (257: the stride loop's second trip for one thread) and 600 (three trips).  Scores: randn; randn +
    1e4; one frame 120 above the rest - every other weight underflows, none may be NaN or negative; all equal - 1 / t within the bound.
    L = ceil(t / 256) + 6 + 2.  The weights of a chunk sum to 1 within (t / 256 + 10) u.  The backward takes the weights the forward produced."""
    rs = np.random.RandomState(seed_of("softmax", t, family))
    b = 3
    score = softmax_scores(rs, b, t, family)
    w = be.softmax(score)
    form = "softmax_segments%s" % (", stride loop" if t > 256 else "")
    assert np.all(w >= 0) and np.all(np.isfinite(w))
    LEDGER.check(form, "weights (%s)" % family, w, A.softmax(score), A.softmax_bound(score))
    LEDGER.check(form, "sum of a chunk's weights", R.f64(w).sum(axis=1), np.ones(b), A.softmax_sum_bound(t))
    if family == "equal":
        LEDGER.check(form, "equal scores: 1 / t", w, np.full((b, t), 1.0 / t), A.softmax_bound(score))
    if family == "dominant" and t > 1:
        assert np.sort(w, axis=1)[:, -2].max() < 1e-37 and np.all(w.max(axis=1) == 1.0)
    dw = R.f32(rs.randn(b, t) * (10.0 ** (np.arange(b) - 1))[:, None])
    ds = be.softmax_backward(w, dw)
    LEDGER.check(form.replace("segments", "segments_backward"), "dscore (%s)" % family, ds, A.softmax_backward(w, dw), A.softmax_backward_bound(w, dw))


@pytest.mark.parametrize("t,family", SOFTMAX_CASES)
def test_softmax_segments(be, t, family):
    row_softmax(be, t, family)


# =========================================================================================== d weights of the pooling
POOL_DW_CASES = [(kind, affine, fam) for kind in G.KINDS for affine in (True, False) for fam in ("base", "hetero")]
POOL_DW_SHAPES = [(3, 1), (3, 5), (3, 33), (4, 5)]      # rows % 4 in {3, 3, 3, 0}


def pooled_vector(rs, b, n, family):
    """[b][2 n] means and standard deviations as a pooling forward would hand them over; chunk 0 carries, in its first channels, the four sides
    of the kernel's sd <= 1e-6 rule: 0, exactly 1e-6f, the next float above it, an ordinary value."""
    cs = R.channel_scale(n) if family == "hetero" else np.ones(n)
    pool = np.concatenate([rs.randn(b, n) * cs, (rs.rand(b, n) + 0.5) * cs], axis=1).astype(np.float32)
    special = [np.float32(0), A.SD_EPS32, np.nextafter(A.SD_EPS32, np.float32(1)), np.float32(0.75)]
    pool[0, n:n + 4] = special[:min(4, n)]
    return pool


def row_att_pool_dw(be, kind, affine, family):
    """att_pool_dw_kernel through xv_att_pool_backward_weights: b x t in {3 x 1, 3 x 5, 3 x 33, 4 x 5} (rows % 4 in {3, 0}: the last block's
    waves without a row), c in {4, 256, 260} around one quad per lane, 2 048 / 2 052 around the second pass; scale / shift given or NULL;
    relu = 0, plain ReLU, a prelu vector of both signs and the constant 0.2 slope through xv_set_activation; the pooled vector is the row's own
    (pooled_vector: all four sides of sd <= 1e-6 in chunk 0).  L = ceil(c / 256) + 2 + 6 (A.pool_dw_chain)."""
    rs = np.random.RandomState(seed_of("pool_dw", kind, affine, family))
    for b, t in POOL_DW_SHAPES:
        for c in (4, 256, 260, 2048, 2052):
            z = R.make_z(rs, b * t, c, family)
            scale, shift = R.make_affine(rs, c, family, negative=1) if affine else (None, None)
            relu, slope, _ = slope_of(rs, kind, c)
            pool, dpool = pooled_vector(rs, b, c, family), R.make_grad(rs, (b, 2 * c), family)
            dv = A.pool_dvar(pool, dpool, c)
            assert np.all(dv[0, :2] == 0) and np.all(dv[0, 2:4] != 0)
            got = be.att_pool_dw(z, b, t, scale, shift, relu, slope, pool, dpool)
            ref = A.att_pool_dw(z, b, t, scale, shift, relu, slope, pool, dpool)
            bound, amb = A.att_pool_dw_bound(z, b, t, scale, shift, relu, slope, pool, dpool)
            form = "att_pool_dw %s%s%s" % (kind, "" if affine else ", no scale / shift", ", second pass" if c > A.SCORE_PASS else "")
            LEDGER.check(form, "dweights", got, ref, bound)
            LEDGER.check(form, "dweights of the chunk with clamped deviations", got[0], ref[0], bound[0])
            note_share(form, "pool_dw %s %s %s %dx%dx%d" % (kind, affine, family, b, t, c), amb)


@pytest.mark.parametrize("kind,affine,family", POOL_DW_CASES)
def test_att_pool_backward_weights(be, kind, affine, family):
    row_att_pool_dw(be, kind, affine, family)


# =========================================================================================== key layer backward
KEY_BWD_CASES = [(act, fam) for act in (0, 1, 3) for fam in ("base", "hetero")]


def row_key_backward(be, act, family):
    """att_key_bwd_kernel + xv_colsum through xv_att_key_backward: rows in {1, 3} (fewer than the 4 row lanes), {63, 64, 65} around the 64-row
    chunk and 130 (three chunks); n in {4, 252, 256, 260} around a block's 64 column quads and 1 500; act = 1 on exact zeros in zk, whose
    derivative is exactly 0; dbias given and, at n = 256, NULL; from 65 rows on the first chunk's dscore is all zero: its dzk is exactly 0.
    L = 16 + 2 + the column sum over the chunks (A.key_bwd_chain)."""
    rs = np.random.RandomState(seed_of("key_bwd", act, family))
    for rows in (1, 3, 63, 64, 65, 130):
        for n in (4, 252, 256, 260, 1500):
            zk, q = A.make_key(rs, rows, n, family, zeros=act == 1)
            scale = 1.0 / np.sqrt(n)
            ds = R.f32(rs.randn(rows) * 0.05)
            if rows > A.AKB_ROWS:
                ds[:A.AKB_ROWS] = 0
            ref = A.key_backward(zk, act, q, scale, ds)
            bounds = list(A.key_backward_bound(zk, act, q, scale, ds))
            if n == 1500 and family == "base" and rows >= 63:      # test_self_attention_pieces: 1e-4 of the largest entry
                bounds[0], bounds[1] = LEDGER.capped(bounds[0], ref[0], 1e-4), LEDGER.capped(bounds[1], ref[1], 1e-4)
            for want_dbias in ((True, False) if n == 256 else (True,)):
                dzk, dq, db = be.key_backward(zk, act, q, scale, ds, want_dbias)
                form = "att_key_backward act %d%s" % (act, "" if want_dbias else ", no dbias")
                LEDGER.check(form, "dzk", dzk, ref[0], bounds[0])
                LEDGER.check(form, "dquery", dq, ref[1], bounds[1])
                if want_dbias:
                    LEDGER.check(form, "dbias", db, ref[2], bounds[2])
                if act == 1:
                    LEDGER.exact(form, "dzk where zk <= 0", dzk[zk <= 0], np.zeros(int((zk <= 0).sum()), np.float32))
                    assert (zk == 0).any()
                if rows > A.AKB_ROWS:
                    LEDGER.exact(form, "dzk of a chunk without gradient", dzk[:A.AKB_ROWS], np.zeros((A.AKB_ROWS, n), np.float32))


@pytest.mark.parametrize("act,family", KEY_BWD_CASES)
def test_att_key_backward(be, act, family):
    row_key_backward(be, act, family)


# =========================================================================================== key_activation, add_inplace
KEY_ACT_CASES = [(count, act) for count in (1, 255, 257, GRID_TRIP + 3) for act in (0, 1, 3)]


def row_key_activation(be, count, act):
    """key_activation_kernel: count in {1, 255, 257} around a block and 8 192 x 256 + 3 - three elements into the second trip of the grid-stride
    loop.  Identity and ReLU bit for bit, tanh within its allowance."""
    rs = np.random.RandomState(seed_of("key_act", count, act))
    z = R.f32(rs.randn(count) * 2)
    z[::7] = 0
    y = be.key_activation(z, act)
    form = "key_activation%s" % (" (grid stride)" if count > GRID_TRIP else "")
    if act == 3:
        LEDGER.check(form, "tanh", y, A.key_act(z, 3), A.key_act_bound(z, 3))
    else:
        LEDGER.exact(form, "act %d" % act, y, A.key_act(z, act, np.float32))


@pytest.mark.parametrize("count,act", KEY_ACT_CASES)
def test_key_activation(be, count, act):
    row_key_activation(be, count, act)


ADD_CASES = [(count, same) for count in (4, 4 * GRID_TRIP + 4) for same in (True, False)]


def row_add_inplace(be, count, same):
    """add_inplace_kernel: one float4, and 8 192 x 256 + 1 float4s - one into the second trip; x == y (doubling) and x != y; bit for bit."""
    rs = np.random.RandomState(seed_of("add", count, same))
    y = R.f32(rs.randn(count))
    x = None if same else R.f32(rs.randn(count) * 3)
    got = be.add_inplace(y, x)
    LEDGER.exact("add_inplace%s" % (" (grid stride)" if count > 4 * GRID_TRIP else ""), "x == y" if same else "x != y", got, y + (y if same else x))


@pytest.mark.parametrize("count,same", ADD_CASES)
def test_add_inplace(be, count, same):
    row_add_inplace(be, count, same)


# =========================================================================================== refusals, by name
def test_refusals(be):
    from tf_kaldi_speaker_amd._lib import XvError
    t, p, s = be.torch, be.ops._p, be.stream()
    buf = t.zeros(1024, dtype=t.float32, device=be.dev_name)
    zk, dzk, q, dq, ds = buf[:256].view(64, 4), buf[256:512].view(64, 4), buf[512:516], buf[516:520], buf[520:584]
    with pytest.raises(XvError, match="att_key_backward: workspace too small"):
        be.lib.call("xv_att_key_backward", s, p(zk), 64, 4, 0, p(q), 1.0, p(ds), p(dzk), p(dq), None, p(buf), C.c_size_t(16))
    with pytest.raises(XvError, match="att_key_backward: bad arguments"):
        be.lib.call("xv_att_key_backward", s, p(zk), 64, 4, 2, p(q), 1.0, p(ds), p(dzk), p(dq), None, p(buf), C.c_size_t(1 << 20))
    with pytest.raises(XvError, match="key_activation: act must be 0"):
        be.lib.call("xv_key_activation", s, p(zk), C.c_size_t(8), 2, p(dzk))
    with pytest.raises(XvError, match="add_inplace: count and pointers must be 16-byte multiples"):
        be.lib.call("xv_add_inplace", s, p(buf), p(buf), C.c_size_t(6))
    with pytest.raises(XvError, match="add_inplace: count and pointers must be 16-byte multiples"):
        be.lib.call("xv_add_inplace", s, p(buf[1:]), p(buf), C.c_size_t(8))
    with pytest.raises(XvError, match="add_inplace: count and pointers must be 16-byte multiples"):
        be.lib.call("xv_add_inplace", s, p(buf), p(buf[3:]), C.c_size_t(8))
    with pytest.raises(XvError, match="att_score: bad arguments"):
        be.lib.call("xv_att_score", s, p(zk), 64, 4, 3, 0, p(q), 1.0, p(ds))      # a pitch under the row length
    t.cuda.synchronize()
    assert float(buf.abs().sum().item()) == 0.0      # nothing was launched
