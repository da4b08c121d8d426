"""NumPy restatement of the self-attention kernels (csrc/xv_attention.hip: score, softmax over frames and its backward, d weights of the
weighted pooling, the key layer's backward, key_activation, add_inplace) with the rounding bound of each output, what
tests/test_gpu_attention_forms.py compares the kernels with.

As in tests/bn_pool_ref.py: every formula takes a dtype, float64 is the reference and float32 the plain NumPy evaluation that
tests/test_attention_ref.py holds against the same bounds before a kernel runs (class NumpyOps); u = 2^-24; a sum of terms t_i with a longest
addition chain of L and c roundings per term is within (L + c) u sum|t_i| of the exact sum; nothing is relative to a tensor's largest entry.

Transcendental functions.  HIP's math API table gives a maximum error of 1 ulp for expf and 2 ulp for tanhf (no documentation on the build
machine states otherwise); an ulp of x is at most 2 u |x|.  The same allowance again covers NumPy's float32 function in the CPU backend, so
one bound serves both: EXP_REL = 2 * 1 * 2 u, TANH_REL = 2 * 2 * 2 u.  They are allowances stated here, not figures fitted to an output; the
ledger records how much of a bound is used."""
import numpy as np

import bn_pool_ref as R
from bn_pool_ref import U, cdiv, f32, f64

EXP_REL = 2 * 1 * 2 * U        # expf: 1 ulp, device + NumPy
TANH_REL = 2 * 2 * 2 * U       # tanhf: 2 ulp, device + NumPy
FLT_MIN = 2.0 ** -126          # a result under the smallest normal float32 may be flushed to zero
SD_EPS32 = np.float32(1e-6)    # att_pool_dw_kernel: no gradient through a standard deviation at or under it
AKB_ROWS = 64                  # rows per chunk of att_key_bwd_kernel
SCORE_PASS = 2048              # columns one pass of the vector score / d weights loop covers (64 lanes x 8 quads)


# ------------------------------------------------------------------ input families
def channel_scale(n):
    return R.channel_scale(n)


def make_key(rs, rows, n, family="base", zeros=False):
    """Key pre-activations (0.7 randn, as tests/test_gpu_ops.py) and the query (0.1 randn; heterogeneous: channel c times 10^(c mod 7 - 3))."""
    zk = rs.randn(rows, n) * 0.7
    q = rs.randn(n) * 0.1
    if family == "hetero":
        q = q * channel_scale(n)
    if zeros:
        zk[rs.rand(rows, n) < 0.2] = 0.0
        zk.flat[0] = 0.0
    return f32(zk), f32(q)


# ------------------------------------------------------------------ key activation
def key_act(z, act, dt=np.float64):
    """0 identity, 1 relu, 3 tanh."""
    z = np.asarray(z, dtype=dt)
    return np.tanh(z) if act == 3 else (np.maximum(z, dt(0)) if act == 1 else z)


def key_act_bound(z, act):
    """Identity and ReLU are exact; tanh within its allowance."""
    return TANH_REL * np.abs(key_act(z, act)) if act == 3 else np.zeros(np.shape(z))


# ------------------------------------------------------------------ score
def score_chain(n, vector):
    """Vector form: a lane holds quads lane + 64 u; the 4 products of a quad are added as (p0 + p1) + (p2 + p3) (2), the quads of a lane one
    after the other (ceil(n / 4 / 64)), then six butterfly steps.  Scalar form: columns lane + 64 j in order, then the butterfly."""
    return (cdiv(cdiv(n, 4), 64) + 2 + 6) if vector else (cdiv(n, 64) + 6)


def att_score(zk, act, q, scale, dt=np.float64):
    """score[r] = scale * sum_c act(zk[r][c]) q[c]"""
    k = key_act(zk, act, dt)
    return R.rsum(k * np.asarray(q, dtype=dt), 1, dt) * dt(np.float32(scale))


def att_score_bound(zk, act, q, scale, vector):
    """A term carries the activation's error, its product's rounding, and the final product with scale one more: (L + 2) u + tanh's allowance,
    times |scale| sum |act(zk) q|."""
    mag = np.abs(key_act(zk, act) * f64(q)).sum(axis=1) * abs(float(np.float32(scale)))
    return ((score_chain(zk.shape[1], vector) + 2) * U + (TANH_REL if act == 3 else 0.0)) * mag


# ------------------------------------------------------------------ softmax over the frames of a chunk
def softmax_chain(t):
    """A thread adds its ceil(t / 256) elements in order, six butterfly steps, then (w0 + w1) + (w2 + w3) over the waves."""
    return cdiv(t, 256) + 6 + 2


def softmax(score, dt=np.float64):
    s = np.asarray(score, dtype=dt)
    e = np.exp(s - s.max(axis=1, keepdims=True))
    return e / R.rsum(e, 1, dt)[:, None]


def softmax_bound(score):
    """e_i = exp(s_i - m): the difference rounds (u |s_i - m|, which the exponential turns into a relative error of as much) and expf has its
    allowance: eps_i = u |s_i - m| + EXP_REL.  The sum z of the e_j is off by L u z and by sum_j e_j eps_j; the quotient rounds once:
      d w_i = w_i (eps_i + (L + 1) u + sum_j w_j eps_j)  + FLT_MIN (an underflowing weight; z >= 1)."""
    s = f64(score)
    d = np.abs(s - s.max(axis=1, keepdims=True))
    w = softmax(s)
    eps = U * d + EXP_REL
    L = softmax_chain(s.shape[1])
    return w * (eps + (L + 1) * U + (w * eps).sum(axis=1, keepdims=True)) * (1 + 1e-3) + FLT_MIN


def softmax_sum_bound(t):
    """|sum_i w_i - 1|: the weights are e_i / z with the z that the kernel's own chain summed from the same e_i: (L + 1) u for the chain and
    the quotients, one u to spare - (t / 256 + 10) u."""
    return (softmax_chain(t) + 2) * U


def softmax_backward(w, dw, dt=np.float64):
    """ds = w (dw - sum_t w dw)"""
    w, dw = np.asarray(w, dtype=dt), np.asarray(dw, dtype=dt)
    return w * (dw - R.rsum(w * dw, 1, dt)[:, None])


def softmax_backward_bound(w, dw):
    """z = sum w dw: (L + 1) u sum|w dw|; ds = w (dw - z): |w| (d z + u (|dw| + |z|)) + u |ds|."""
    w, dw = f64(w), f64(dw)
    L = softmax_chain(w.shape[1])
    z = (w * dw).sum(axis=1, keepdims=True)
    dz = (L + 1) * U * np.abs(w * dw).sum(axis=1, keepdims=True)
    return np.abs(w) * (dz + U * (np.abs(dw) + np.abs(z))) + U * np.abs(w * (dw - z))


# ------------------------------------------------------------------ d weights of the weighted statistics pooling
def pool_dw_chain(n):
    """As the vector score: (v0 + v1) + (v2 + v3) per quad, a lane's quads in order, six butterfly steps."""
    return cdiv(cdiv(n, 4), 64) + 2 + 6


def pool_dvar(pool, dpool, n, dt=np.float64):
    """dvar = dstd 0.5 / std, 0 where the float32 std is at or under float32 1e-6 - the comparison the kernel makes, on the pooled vector as handed in."""
    po, dp = np.asarray(pool, dtype=dt), np.asarray(dpool, dtype=dt)
    off = f32(pool)[:, n:] <= SD_EPS32
    return np.where(off, dt(0), dp[:, n:] * dt(0.5) / np.where(off, dt(1), po[:, n:]))


def att_pool_dw(z, b, t, scale, shift, relu, slope, pool, dpool, dt=np.float64):
    """dw[b][t] = sum_c dmean[c] a + dvar[c] (a - mean[c])^2,  a = act(z scale + shift) (scale None: a = act(z))"""
    z = np.asarray(z, dtype=dt)
    n = z.shape[1]
    y = z if scale is None else z * np.asarray(scale, dtype=dt) + np.asarray(shift, dtype=dt)
    a = R.act(y, relu, slope, dt).reshape(b, t, n)
    po, dp = np.asarray(pool, dtype=dt), np.asarray(dpool, dtype=dt)
    dv = pool_dvar(pool, dpool, n, dt)
    cen = a - po[:, None, :n]
    return R.rsum(dp[:, None, :n] * a + dv[:, None] * cen * cen, 2, dt)


def att_pool_dw_bound(z, b, t, scale, shift, relu, slope, pool, dpool):
    """a is within d_a = 2 u (|z scale| + |shift|) max(1, |slope|) + u |a| (R.bn_apply_bound; 0 without scale and slope); the first term dm a then
    carries 1 rounding, the second - dvar (division, 2 with one to spare), the centring (twice, it is squared), two products - 6, their sum 1:
      (L + 8) u sum_c (|dm a| + |dv cen^2|) + sum_c (|dm| + 2 |dv cen|) d_a
    A mask-ambiguous element may take the other branch of the activation: |1 - slope| |y| more in a (|y| itself for plain ReLU).
    -> bound [b][t], ambiguous mask [b t][n]"""
    z = f64(z)
    n = z.shape[1]
    if scale is None:
        y, mag, amb = z, np.zeros_like(z), np.zeros(z.shape, bool)
    else:
        y, _, amb, mag = R.pre_activation(z, scale, shift)
    sl = np.zeros(n) if slope is None else f64(slope)
    a = R.act(y, relu, slope)
    d_a = 2 * U * mag * R.slope_mag(relu, slope, n) + (U * np.abs(a) if (slope is not None and relu) else 0.0)
    if relu:
        d_a = d_a + np.where(amb, np.abs(1 - sl) * np.abs(y), 0.0)
    else:
        amb = np.zeros(z.shape, bool)
    po, dp = f64(pool), f64(dpool)
    dv = pool_dvar(pool, dpool, n)
    a3, d_a3 = a.reshape(b, t, n), np.broadcast_to(d_a, z.shape).reshape(b, t, n)
    cen = a3 - po[:, None, :n]
    t1, t2 = np.abs(dp[:, None, :n] * a3), np.abs(dv[:, None] * cen * cen)
    lin = (np.abs(dp[:, None, :n]) + 2 * np.abs(dv[:, None] * cen)) * d_a3 + np.abs(dv[:, None]) * d_a3 ** 2
    return (pool_dw_chain(n) + 8) * U * (t1 + t2).sum(axis=2) + lin.sum(axis=2), amb


# ------------------------------------------------------------------ key layer backward
def colsum_chain(rows):
    """xv_colsum: a row lane of colsum_partial_kernel adds at most 32 rows of its 128-row chunk (in fours: at most 8 + 3 additions, counted as
    min(ceil(rows / 4), 32)), the 4 lanes (2); colsum_final_kernel: a lane's ceil(chunks / 8) partials, then the 8 lanes in order."""
    return min(cdiv(rows, 4), 32) + 2 + cdiv(cdiv(rows, 128), 8) + 8


def key_bwd_chain(rows):
    """att_key_bwd_kernel: a row lane adds its at most 16 rows of the 64-row chunk in row order, (l0 + l1) + (l2 + l3), then xv_colsum over the chunks."""
    return 16 + 2 + colsum_chain(cdiv(rows, AKB_ROWS))


def key_backward(zk, act, q, scale, ds, dt=np.float64):
    """dzk[r][c] = ds[r] scale q[c] act'(zk[r][c]);  dq[c] = scale sum_r ds[r] act(zk[r][c]);  dbias[c] = sum_r dzk[r][c]"""
    zk, q, ds = np.asarray(zk, dtype=dt), np.asarray(q, dtype=dt), np.asarray(ds, dtype=dt).reshape(-1, 1)
    sc = dt(np.float32(scale))
    k = key_act(zk, act, dt)
    dk = (dt(1) - k * k) if act == 3 else ((zk > 0).astype(dt) if act == 1 else np.ones_like(zk))
    dzk = (q * sc) * ds * dk
    return dzk, R.rsum(k * ds, 0, dt) * sc, R.rsum(dzk, 0, dt)


def key_backward_bound(zk, act, q, scale, ds):
    """dzk: q scale, times ds, times act' - 3 roundings - and act' = 1 - k^2 with k = tanh within TANH_REL |k|: d act' = (2 TANH_REL + u) k^2 + u act'
    (identity and ReLU: act' is exactly 1 or 0, the ReLU mask is taken from the input itself).
    dq: a term k ds carries tanh's allowance and its product, the chunk sum is multiplied by scale: (L + 2) u + TANH_REL.
    dbias adds the float32 dzk: L u sum|dzk| + sum d dzk."""
    zk, q, ds = f64(zk), f64(q), f64(ds).reshape(-1, 1)
    sc = abs(float(np.float32(scale)))
    k = key_act(zk, act)
    dzk, _, _ = key_backward(zk, act, q, scale, ds)
    head = np.abs(q * sc * ds)
    b_dzk = 3 * U * np.abs(dzk) + (head * ((2 * TANH_REL + U) * k * k + U * (1 - k * k)) if act == 3 else 0.0)
    L = key_bwd_chain(zk.shape[0])
    b_dq = ((L + 2) * U + (TANH_REL if act == 3 else 0.0)) * np.abs(k * ds).sum(axis=0) * sc
    b_db = L * U * np.abs(dzk).sum(axis=0) + (b_dzk * np.ones_like(zk)).sum(axis=0)
    return b_dzk * np.ones_like(zk), b_dq, b_db


# ------------------------------------------------------------------ the same interface as the GPU backend, in plain float32 NumPy
class NumpyOps(object):
    name = "numpy-float32"
    dt = np.float32

    def att_score(self, zk, act, q, scale, ldz=None, offset=0, want_form=None):
        return f32(att_score(zk, act, q, scale, self.dt))

    def softmax(self, score):
        return f32(softmax(score, self.dt))

    def softmax_backward(self, w, dw):
        return f32(softmax_backward(w, dw, self.dt))

    def att_pool_dw(self, z, b, t, scale, shift, relu, slope, pool, dpool):
        return f32(att_pool_dw(z, b, t, scale, shift, relu, slope, pool, dpool, self.dt))

    def key_backward(self, zk, act, q, scale, ds, want_dbias=True):
        dzk, dq, db = key_backward(zk, act, q, scale, ds, self.dt)
        return f32(dzk), f32(dq), (f32(db) if want_dbias else None)

    def key_activation(self, z, act):
        return f32(key_act(z, act, self.dt))

    def add_inplace(self, y, x=None):
        y = f32(y)
        return y + (y if x is None else f32(x))
