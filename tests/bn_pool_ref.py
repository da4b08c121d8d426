"""NumPy restatement of the BatchNorm, statistics-pooling and l2_scaling ops (csrc/xv_bn.hip, xv_bn_bwd.hip, xv_pool.hip) with the
rounding bound of each output, what tests/test_gpu_bn_pool_forms.py compares the kernels with.

Every formula takes a dtype: float64 is the reference, float32 is the plain NumPy evaluation tests/test_bn_pool_ref.py holds against
the same bounds before any kernel runs (class NumpyOps below has the interface of the GPU backend of the rows).  The oracle
(oracle/xvector_oracle.py) composes whole layers in float64; a kernel in isolation is compared here with its own operation on the
float32 parameter vectors it was handed (mean, invstd, scale, shift, pooled statistics, wpos), which the row of the kernel that
produces them checks.

Bounds.  u = 2^-24.  A sum of terms t_i in a fixed order with a longest addition chain of L and c roundings per term is within
(L + c) u sum|t_i| of the exact sum of the exact terms; an element-wise result within c u times the magnitudes of the operands of its
last addition.  L is stated by the rows (derived from the kernels' loops), c here beside each formula.  Nothing is relative to a
tensor's largest entry.

Masks.  ReLU / slope masks come from y = z * scale + shift in float64 with the float32 scale and shift; an element with
|y| <= 16 u (|z scale| + |shift|) is ambiguous: it is left out of element-wise comparisons and its possible contribution is added to
the bound of every reduction it feeds."""
import numpy as np

U = 2.0 ** -24
TILE_M = 128
VAR_EPS = 1e-12                # pooling.py:28-29 variance clamp
AMBIGUOUS = 16.0               # |y| <= AMBIGUOUS u (|z scale| + |shift|)
MAX_AMBIGUOUS_SHARE = 1e-4


def f64(a):
    return None if a is None else np.asarray(a, dtype=np.float64)


def f32(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float32)


def cdiv(a, b):
    return (a + b - 1) // b


def rsum(x, axis, dt):
    """Sum over one axis with NumPy's pairwise order (the axis made the last, contiguous one): a plain sum over a leading axis adds slice by
    slice, a chain as long as the axis - longer than any of the kernels'."""
    return np.ascontiguousarray(np.moveaxis(np.asarray(x), axis, -1)).sum(axis=-1, dtype=dt)


# ------------------------------------------------------------------ input families
def channel_scale(n):
    """The heterogeneous family: channel c carries 10^(c mod 7 - 3)."""
    return 10.0 ** (np.arange(n) % 7 - 3.0)


def make_z(rs, rows, n, family="base"):
    if family == "offset":
        return f32(1000.0 + rs.randn(rows, n))
    z = rs.randn(rows, n) * 2 + 0.3
    if family == "hetero":
        z = z * channel_scale(n)
    return f32(z)


def make_affine(rs, n, family="base", negative=None):
    """gamma in [0.5, 1.5), beta = 0.3 randn; heterogeneous: both scaled by the channel scale shifted by three channels."""
    gamma, beta = rs.rand(n) + 0.5, 0.3 * rs.randn(n)
    if family == "hetero":
        s = np.roll(channel_scale(n), 3)
        gamma, beta = gamma * s, beta * s
    if negative is not None and negative < n:
        gamma[negative] = -gamma[negative]
    return f32(gamma), f32(beta)


def make_grad(rs, shape, family="base"):
    g = rs.randn(*shape)
    if family == "hetero":
        g = g * np.roll(channel_scale(shape[-1]), 5)
    return f32(g)


# ------------------------------------------------------------------ comparison
def worst_ratio(got, ref, bound, keep=None):
    """max |got - ref| / bound over the kept elements; where the bound is 0 the values must be equal (ratio 0, else inf)."""
    got, ref, bound = f64(got), f64(ref), f64(bound)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    bound = np.broadcast_to(bound, ref.shape)
    assert np.all(np.isfinite(got)), "non-finite output"
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    if keep is not None:
        r = np.where(keep, r, 0.0)
    return float(r.max()) if r.size else 0.0


class Ledger(object):
    """The largest ratio to its bound per form, over the rows that ran."""

    def __init__(self):
        self.worst = {}

    def check(self, form, name, got, ref, bound, keep=None):
        r = worst_ratio(got, ref, bound, keep)
        key = "%s / %s" % (form, name)
        self.worst[key] = max(self.worst.get(key, 0.0), r)
        assert r <= 1.0, "%s: error is %.3g x its bound" % (key, r)
        return r

    def exact(self, form, name, got, ref):
        got, ref = np.asarray(got), np.asarray(ref)
        key = "%s / %s (exact)" % (form, name)
        ok = got.shape == ref.shape and np.array_equal(got, ref)
        self.worst[key] = max(self.worst.get(key, 0.0), 0.0 if ok else np.inf)
        assert ok, "%s: not bit-equal (largest difference %.3g)" % (key, np.abs(f64(got) - f64(ref)).max())

    @staticmethod
    def capped(bound, ref, rel):
        """The tolerance of the row of tests/test_gpu_ops.py that a row supplements - rel times the tensor's largest entry - stays a ceiling:
        the derived bound wherever it is tighter, never more than that."""
        return np.minimum(bound, rel * np.abs(f64(ref)).max())

    def lines(self):
        return ["%-64s %8.4f" % (k, v) for k, v in sorted(self.worst.items())]


# ------------------------------------------------------------------ activation
def pre_activation(z, scale, shift):
    """y in float64, the on mask and the ambiguous mask."""
    z, scale, shift = f64(z), f64(scale), f64(shift)
    y = z * scale + shift
    mag = np.abs(z * scale) + np.abs(shift)
    return y, y > 0, np.abs(y) <= AMBIGUOUS * U * mag, mag


def act(y, relu, slope, dt=np.float64):
    """relu ? (y > 0 ? y : slope * y) : y; slope None = plain ReLU."""
    if not relu:
        return y
    neg = np.zeros_like(y) if slope is None else y * np.asarray(slope, dtype=dt)
    return np.where(y > 0, y, neg)


def slope_mag(relu, slope, n):
    """max(1, |slope|) per channel: how much the activation can stretch an error of y."""
    return np.ones(n) if (not relu or slope is None) else np.maximum(1.0, np.abs(f64(slope)))


def fma32(a, b, c):
    """float32 fma: the product of two float32 is exact in float64, the sum is rounded there (53 bits) and once more to float32."""
    return (f64(a) * f64(b) + f64(c)).astype(np.float32)


# ------------------------------------------------------------------ col_stats / bn_finalize / bn_output_range / bn_inference_scale
COL_STATS_L = 16 + 8           # a thread's 16 rows of the tile in row order, then the 8 row lanes in lane order (both forms)


def tiles_of(rows):
    return cdiv(rows, TILE_M)


def col_stats(z, dt=np.float64):
    """[4][tiles][n]: per 128-row tile the sum, the squares centred on the tile mean (sum / count, in dt), min, max."""
    z = np.asarray(z, dtype=dt)
    rows, n = z.shape
    out = np.zeros((4, tiles_of(rows), n), dt)
    for t in range(out.shape[1]):
        blk = z[t * TILE_M:(t + 1) * TILE_M]
        s = rsum(blk, 0, dt)
        m = s / dt(blk.shape[0])
        out[0, t], out[1, t], out[2, t], out[3, t] = s, rsum((blk - m) ** 2, 0, dt), blk.min(axis=0), blk.max(axis=0)
    return out


def col_stats_bound(z, L=COL_STATS_L):
    """Sum: terms are exact, L u S.  Squares: the kernel centres on its float32 tile mean m^, off the true mean m by at most
    dm = bound(sum) / count + u |m| (the division); sum (z - m^)^2 = sum (z - m)^2 + count (m - m^)^2 exactly (the cross term vanishes about the
    true mean), and a term (z - m^)^2 carries 3 roundings: (L + 3) u Q + count dm^2.  -> (bound [2][tiles][n], dm [tiles][n])
    L: the longest addition chain of the kernel that forms the statistics (xv_col_stats by default; the GEMM epilogues state their own)."""
    z = f64(z)
    rows, n = z.shape
    T = tiles_of(rows)
    b, dm = np.zeros((2, T, n)), np.zeros((T, n))
    for t in range(T):
        blk = z[t * TILE_M:(t + 1) * TILE_M]
        cnt = blk.shape[0]
        m = blk.mean(axis=0)
        b[0, t] = L * U * np.abs(blk).sum(axis=0)
        dm[t] = b[0, t] / cnt + U * np.abs(m)
        b[1, t] = (L + 3) * U * ((blk - m) ** 2).sum(axis=0) * (1 + 1e-3) + cnt * dm[t] ** 2
    return b, dm


def bn_finalize(part, rows, gamma, beta, eps, momentum, unbiased, mm, mv, dt=np.float64):
    """The finalisation from the partials: count-weighted merge of the tile means and centred squares (the kernel: Chan's formula in double),
    biased variance, invstd, scale, shift, moving statistics."""
    part = np.asarray(part, dtype=dt)
    T = part.shape[1]
    tc = np.minimum(TILE_M, rows - TILE_M * np.arange(T)).astype(dt)[:, None]
    tm = part[0] / tc
    mean = rsum(tm * tc, 0, dt) / dt(rows)
    var = (rsum(part[1], 0, dt) + rsum(tc * (tm - mean) ** 2, 0, dt)) / dt(rows)
    invstd = dt(1) / np.sqrt(var + dt(np.float32(eps)))
    scale = np.asarray(gamma, dtype=dt) * invstd
    shift = np.asarray(beta, dtype=dt) - mean * scale
    out = dict(mean=mean, invstd=invstd, scale=scale, shift=shift, zmin=part[2].min(axis=0), zmax=part[3].max(axis=0))
    if mm is not None:
        om = dt(np.float32(1) - np.float32(momentum))
        v = var * (dt(rows) / dt(rows - 1)) if (unbiased and rows > 1) else var
        out["moving_mean"] = np.asarray(mm, dtype=dt) * dt(np.float32(momentum)) + mean * om
        out["moving_var"] = np.asarray(mv, dtype=dt) * dt(np.float32(momentum)) + v * om
    return out


def bn_finalize_truth(z, gamma, beta, eps, momentum, unbiased, mm, mv):
    """What col_stats + bn_finalize compute, from z in float64 (the float32 gamma, beta, moving buffers as given), and the bound of each output.

    mean: the tile sums are off by L u S_t (col_stats), a tile mean by one more rounding, the merge runs in double and the result is cast:
      d mean = (L + 2) u sum|z| / rows.
    var: with m^_t the float32 tile mean the partial squares are centred on, M the merged mean and m_t the true tile mean,
      sum (z - M)^2 = sum_t [ Q_t + 2 (m^_t - M) count_t (m_t - m^_t) + count_t (m^_t - M)^2 ]
    and the kernel leaves the middle (cross) term out - it takes m^_t for the tile's true mean:
      rows d var = (L + 3) u sum_t Q_t + 2 sum_t (|m_t - mean| + dm_t + d mean) count_t dm_t + rows (d mean)^2,   then one cast (2 u var).
    invstd = 1 / sqrt(var + eps): 1/2 invstd^3 (d var + u (var + eps)) + 3 u invstd (sqrt, division, and one to spare).
    scale = gamma invstd: |gamma| d invstd + u |scale|.   shift = beta - mean scale: |scale| d mean + |mean| d scale + 2 u (|beta| + |mean scale|).
    moving = old momentum + new (1 - momentum) with the float32 (1 - momentum): (1 - momentum) d new + 2 u (|old momentum| + |new (1 - momentum)|);
    the unbiased variance adds two roundings (2 u) to d new."""
    z, gamma, beta = f64(z), f64(gamma), f64(beta)
    rows, n = z.shape
    eps = float(np.float32(eps))
    mean = z.mean(axis=0)
    var = ((z - mean) ** 2).mean(axis=0)
    sb, dm = col_stats_bound(z)
    d_mean = (COL_STATS_L + 2) * U * np.abs(z).sum(axis=0) / rows
    cross = np.zeros(n)
    for t in range(dm.shape[0]):
        blk = z[t * TILE_M:(t + 1) * TILE_M]
        cross += 2 * (np.abs(blk.mean(axis=0) - mean) + dm[t] + d_mean) * blk.shape[0] * dm[t]
    d_var = (sb[1].sum(axis=0) + cross + rows * d_mean ** 2) / rows + 2 * U * var
    invstd = 1.0 / np.sqrt(var + eps)
    d_invstd = 0.5 * invstd ** 3 * (d_var + U * (var + eps)) * (1 + 1e-3) + 3 * U * invstd
    scale = gamma * invstd
    d_scale = np.abs(gamma) * d_invstd + U * np.abs(scale)
    shift = beta - mean * scale
    d_shift = np.abs(scale) * d_mean + np.abs(mean) * d_scale + 2 * U * (np.abs(beta) + np.abs(mean * scale))
    ref = dict(mean=mean, invstd=invstd, scale=scale, shift=shift, zmin=z.min(axis=0), zmax=z.max(axis=0))
    bound = dict(mean=d_mean, invstd=d_invstd, scale=d_scale, shift=d_shift)
    if mm is not None:
        mom = float(np.float32(momentum))
        om = float(np.float32(1) - np.float32(momentum))
        unb = unbiased and rows > 1
        v = var * rows / (rows - 1.0) if unb else var
        d_v = d_var * (rows / (rows - 1.0) if unb else 1.0) + (2 * U * v if unb else 0.0)
        ref["moving_mean"] = f64(mm) * mom + mean * om
        ref["moving_var"] = f64(mv) * mom + v * om
        bound["moving_mean"] = om * d_mean + 2 * U * (np.abs(f64(mm) * mom) + np.abs(mean * om))
        bound["moving_var"] = om * d_v + 2 * U * (np.abs(f64(mv) * mom) + np.abs(v * om))
    return ref, bound


def output_range_amax(zmin, zmax, scale, shift, relu, slope):
    """The float32 formula of bn_finalize_kernel / bn_output_range_kernel for the largest |act(z scale + shift)| over the batch: an affine
    (piecewise linear through 0) map has its extremes at the ends, y0 = fma(zmin, scale, shift), y1 = fma(zmax, scale, shift);
    no activation: max(|y0|, |y1|); ReLU: max(0, y0, y1); a slope: max(|act(y0)|, |act(y1)|) with act(y) = y > 0 ? y : y * slope in float32.
    -> the maximum over the channels (the kernels atomicMax the bit patterns of non-negative floats)."""
    y0, y1 = fma32(zmin, scale, shift), fma32(zmax, scale, shift)
    if not relu:
        am = np.maximum(np.abs(y0), np.abs(y1))
    elif slope is None:
        am = np.maximum(np.float32(0), np.maximum(y0, y1))
    else:
        sl = f32(slope)
        a0, a1 = np.where(y0 > 0, y0, y0 * sl), np.where(y1 > 0, y1, y1 * sl)
        am = np.maximum(np.abs(a0), np.abs(a1))
    return np.float32(am.max())


def bn_inference_scale(gamma, beta, mm, mv, eps, dt=np.float64):
    scale = np.asarray(gamma, dtype=dt) * (dt(1) / np.sqrt(np.asarray(mv, dtype=dt) + dt(np.float32(eps))))
    return scale, np.asarray(beta, dtype=dt) - np.asarray(mm, dtype=dt) * scale


def bn_inference_scale_bound(gamma, beta, mm, mv, eps):
    """scale: addition, sqrt, division, product: 4 roundings, 5 u |scale| with one to spare; shift: |mean| d scale + 2 u (|beta| + |mean scale|)."""
    scale, _ = bn_inference_scale(gamma, beta, mm, mv, eps)
    d_scale = 5 * U * np.abs(scale)
    return d_scale, np.abs(f64(mm)) * d_scale + 2 * U * (np.abs(f64(beta)) + np.abs(f64(mm) * scale))


def bn_apply(z, scale, shift, relu, slope, dt=np.float64):
    y = np.asarray(z, dtype=dt) * np.asarray(scale, dtype=dt) + np.asarray(shift, dtype=dt)
    return act(y, relu, slope, dt)


def bn_apply_bound(z, scale, shift, relu, slope):
    """y = z scale + shift: 2 u (|z scale| + |shift|) (product and addition; less as an fma); the activation is 1-Lipschitz (max(1, |slope|) with
    a slope) and the slope's product rounds once more: + u |result|."""
    _, _, _, mag = pre_activation(z, scale, shift)
    return 2 * U * mag * slope_mag(relu, slope, mag.shape[1]) + U * np.abs(bn_apply(z, scale, shift, relu, slope))


# ------------------------------------------------------------------ BatchNorm backward
def finalize_chain(chunks):
    """bn_bwd_finalize_kernel: a lane adds its ceil(chunks / 32) partials in chunk order, lane 0 then adds the 32 lanes in lane order."""
    return cdiv(chunks, 32) + 32


PLAIN_BLOCK_L = 16 + 2         # bn_bwd_reduce_kernel: 16 rows of the 64-row chunk per thread in row order, then (lane0 + lane1) + (lane2 + lane3)
POOLED_BLOCK_L = 16 + 2        # bn_bwd_reduce_pooled_kernel: at most 16 rows of the at most 64-row block per thread, the same lane combine


def closed_chain(b):
    """bn_bwd_pooled_stats_kernel: a lane adds its ceil(b / 64) chunks in order, lane 0 then adds the 64 lanes in lane order."""
    return cdiv(b, 64) + 64


def pool_coef(pool_out, dpool, n):
    """mean, dm, q = dstd / std (0 where the forward clamped: the float32 std <= float32 1e-6), std - per chunk, float64 of the float32 values."""
    po, dp = f64(pool_out), f64(dpool)
    sd32 = f32(pool_out)[:, n:]
    q = np.where(sd32 <= np.float32(1e-6), 0.0, dp[:, n:] / np.where(po[:, n:] == 0, 1.0, po[:, n:]))
    return po[:, :n], dp[:, :n], q, po[:, n:]


def bn_backward(z, gamma, mean, invstd, scale, shift, relu, slope, L, da=None, pooled=None, dt=np.float64):
    """Both reductions, the prelu statistic and the pieces of dz of the BatchNorm (+ activation) backward, from the parameter vectors as given.

    da: the upstream gradient in memory, or pooled = (pool_out, dpool, t, weights or None): the pooling backward on the fly,
      raw = w (dm + q (a - mean_p)),  a = act(y),  w = 1 / t or the frame's weight.
    dd = raw where the unit is on, raw * slope where it is off (0 for plain ReLU);  xhat = (z - mean) invstd
    dbeta = sum dd,  dgamma = sum dd xhat,  dalpha = sum raw min(y, 0)
    -> dict(dd, xhat, raw, dbeta, dgamma, dalpha, ambiguous, and in float64 the bounds b_dbeta, b_dgamma, b_dalpha, raw_mag)

    Bounds (float64 only).  A term of dbeta carries 1 rounding (the slope's product), of dgamma 4 (subtraction, two products, the slope's), of
    dalpha 1 plus the error of y, 2 u (|z scale| + |shift|), on the elements that may be negative.  Pooled: raw is formed with 6 roundings
    relative to raw_mag = w (|dm| + |q| (|z scale| + |shift| + |mean_p|)) max(1, |slope|), which also covers the error of y inside a.  An
    ambiguous element may sit on the other side of the mask: |raw| |1 - slope| more, times |xhat| for dgamma."""
    z = np.asarray(z, dtype=dt)
    rows, n = z.shape
    mu, istd, sc, sh = (np.asarray(v, dtype=dt) for v in (mean, invstd, scale, shift))
    y = z * sc + sh
    sl = np.zeros(n, dt) if slope is None else np.asarray(slope, dtype=dt)
    raw_mag = None
    if pooled is None:
        raw = np.asarray(da, dtype=dt)
    else:
        pool_out, dpool, t, w = pooled
        pm, dm, q, _ = pool_coef(pool_out, dpool, n)
        b = rows // t
        wf = np.full((b, t), dt(1) / dt(t), dt) if w is None else np.asarray(w, dtype=dt).reshape(b, t)
        rep = lambda v: np.repeat(np.asarray(v, dtype=dt), t, axis=0)
        a = act(y, relu, slope, dt)
        wcol = wf.reshape(-1, 1)
        raw = rep(dm) * wcol + (rep(q) * wcol) * (a - rep(pm))
        if dt is np.float64:
            raw_mag = np.abs(wcol) * (np.abs(rep(dm)) + np.abs(rep(q)) * (np.abs(z * sc) + np.abs(sh) + np.abs(rep(pm)))) * slope_mag(relu, slope, n)
    dd = np.where(y > 0, raw, raw * sl) if relu else raw
    xhat = (z - mu) * istd
    out = dict(dd=dd, xhat=xhat, raw=raw, y=y, dbeta=rsum(dd, 0, dt), dgamma=rsum(dd * xhat, 0, dt))
    with_alpha = relu and slope is not None
    if with_alpha:
        out["dalpha"] = rsum(raw * np.minimum(y, 0), 0, dt)
    if dt is np.float64:
        _, _, amb, mag = pre_activation(z, scale, shift)
        amb = amb if relu else np.zeros_like(amb)
        jump = np.where(amb, np.abs(raw) * np.abs(1 - sl), 0.0)
        d_raw = 0.0 if raw_mag is None else 6 * U * raw_mag
        out["ambiguous"] = amb
        out["raw_mag"] = raw_mag
        out["j_dbeta"], out["j_dgamma"] = jump.sum(axis=0), (jump * np.abs(xhat)).sum(axis=0)
        out["b_dbeta"] = (L + 1) * U * np.abs(dd).sum(axis=0) + (d_raw * np.ones_like(z)).sum(axis=0) + jump.sum(axis=0)
        out["b_dgamma"] = (L + 4) * U * np.abs(dd * xhat).sum(axis=0) + (d_raw * np.abs(xhat)).sum(axis=0) + (jump * np.abs(xhat)).sum(axis=0)
        if with_alpha:
            maybe_neg = y <= 2 * U * mag
            out["b_dalpha"] = ((L + 1) * U * np.abs(raw * np.minimum(y, 0)).sum(axis=0) + (d_raw * np.abs(np.minimum(y, 0))).sum(axis=0)
                               + np.where(maybe_neg, np.abs(raw) * 2 * U * mag, 0.0).sum(axis=0))
    return out


def bn_backward_dz(red, z, gamma, mean, invstd, dbeta, dgamma, dt=np.float64):
    """dz = gamma invstd (dd - c1 - xhat c2) with c1 = dbeta / rows, c2 = dgamma / rows of the reductions as given (the kernel's own, which
    their row checks).  Bound (float64): every operand of the last subtraction and what forms it, 10 u |gamma invstd| (raw_mag or |dd|, + |c1| +
    |invstd c2| (|z| + |mean|)); raw_mag in place of |dd| for the pooled forms, whose dense kernel regroups the sum as w (A z + B) + (C z + D)."""
    rows = z.shape[0]
    g_is = np.asarray(gamma, dtype=dt) * np.asarray(invstd, dtype=dt)
    c1, c2 = np.asarray(dbeta, dtype=dt) / dt(rows), np.asarray(dgamma, dtype=dt) / dt(rows)
    dz = g_is * (red["dd"] - c1 - red["xhat"] * c2)
    if dt is not np.float64:
        return dz, None
    head = np.abs(red["dd"]) if red.get("raw_mag") is None else red["raw_mag"]
    bound = 10 * U * np.abs(g_is) * (head + np.abs(c1) + np.abs(f64(invstd) * c2) * (np.abs(f64(z)) + np.abs(f64(mean))))
    return dz, bound


def pad_rows(dz, segs, t, pad):
    """[segs * t][n] -> [segs * (t + 2 pad)][n] with zero frames around each segment."""
    n = dz.shape[1]
    out = np.zeros((segs, t + 2 * pad, n), dz.dtype)
    out[:, pad:pad + t] = dz.reshape(segs, t, n)
    return out.reshape(-1, n)


def closed_form(pool_out, dpool, wpos, gamma, mean, invstd, scale, shift, rows, dt=np.float64):
    """bn_bwd_pooled_stats_kernel: dbeta = sum_b dm W+ + q mean_p (1 - W+),  dgamma = sum_b [dm (mean_p - beta W+) + q (std^2 - beta mean_p (1 - W+))] / gamma
    with beta = shift + mean scale.  -> dbeta, dgamma (and in float64 their bounds against this very formula).

    Bound: a chunk's dbeta term carries 5 roundings relative to |dm W+| + |q mean_p (1 - W+)|; its dgamma term 8 relative to
    |dm| (|mean_p| + B W+) + |q| (std^2 + B |mean_p| (1 - W+)), B = |shift| + |mean scale| standing for |beta| so that beta's own two roundings are
    covered; the division by gamma rounds once more (u |dgamma|)."""
    n = wpos.shape[1]
    po, dp = np.asarray(pool_out, dtype=dt), np.asarray(dpool, dtype=dt)
    pm, sd, dm = po[:, :n], po[:, n:], dp[:, :n]
    q = np.where(f32(pool_out)[:, n:] <= np.float32(1e-6), dt(0), dp[:, n:] / np.where(sd == 0, dt(1), sd))
    wp = np.asarray(wpos, dtype=dt)
    off = dt(1) - wp
    g, mu, sc, sh = (np.asarray(v, dtype=dt) for v in (gamma, mean, scale, shift))
    bt = sh + mu * sc
    dbeta = rsum(dm * wp + q * pm * off, 0, dt)
    dgamma = rsum(dm * (pm - bt * wp) + q * (sd * sd - bt * pm * off), 0, dt) / g
    if dt is not np.float64:
        return dbeta, dgamma, None, None
    L = closed_chain(po.shape[0])
    B = np.abs(sh) + np.abs(mu * sc)
    b1 = (L + 5) * U * (np.abs(dm * wp) + np.abs(q * pm * off)).sum(axis=0)
    b2 = (L + 8) * U * (np.abs(dm) * (np.abs(pm) + B * np.abs(wp)) + np.abs(q) * (sd * sd + B * np.abs(pm * off))).sum(axis=0) / np.abs(g) + U * np.abs(dgamma)
    return dbeta, dgamma, b1, b2


def closed_form_residual(pool_out, dpool, wpos, gamma, mean, scale, shift, d_mean_p, d_std, d_wpos, weights=None):
    """How far the closed form in exact arithmetic can be from the sums over z it replaces, because the pooled statistics it reads are float32
    results with errors of their own (d_mean_p, d_std, d_wpos per chunk and channel: the pooling row's bounds).  With mu, var, W the exact
    pooled mean, variance and active weight of the activation the GPU's scale and shift define, and hats the values handed in,
      sum dd      = dm W + q (mu - mu^ W)                            against  dm W^ + q mu^ (1 - W^)
      sum dd xhat = [dm (mu - beta W) + q (var + mu^2 - mu^ mu - beta (mu - mu^ W))] / gamma^   against the formula on the hats,
    gamma^ = scale / invstd (one rounding from gamma).  First-order in the errors, plus their squares.  The closed form also takes the frame
    weights of a chunk to sum to 1: float32 attention weights sum to n_b = 1 + O(u), and the sums over z are n_b times the expressions above."""
    n = wpos.shape[1]
    pm, dm, q, sd = pool_coef(pool_out, dpool, n)
    B = np.abs(f64(shift)) + np.abs(f64(mean) * f64(scale))
    wp = np.abs(f64(wpos))
    dn = 0.0 if weights is None else np.abs(f64(weights).reshape(pm.shape[0], -1).sum(axis=1) - 1.0)[:, None]
    r1 = ((np.abs(dm) + np.abs(q * pm)) * d_wpos + np.abs(q) * d_mean_p + dn * (np.abs(dm) * wp + np.abs(q * pm) * (1 + wp))).sum(axis=0)
    r2 = (np.abs(dm) * (d_mean_p + B * d_wpos)
          + np.abs(q) * (2 * sd * d_std + d_std ** 2 + (np.abs(pm) + B) * d_mean_p * 2 + d_mean_p ** 2 + B * np.abs(pm) * d_wpos)
          + (2 * U + dn) * (np.abs(dm) * (np.abs(pm) + B) + np.abs(q) * (sd * sd + 2 * pm * pm + 2 * B * np.abs(pm)))).sum(axis=0) / np.abs(f64(gamma))      # last line: gamma^ against gamma, n_b against 1
    return r1, r2


# ------------------------------------------------------------------ statistics pooling
def pool_chain(t):
    """stat_pool_fwd_kernel: a frame lane folds its ceil(t / 4) frames one after the other (two chains over alternate frames in the unrolled
    part), then one merge of the chains and three of the lanes."""
    return cdiv(t, 4) + 4


def stat_pool(a, weights=None, dt=np.float64):
    """[b][t][c] -> mean, std = sqrt(max(var, 1e-12)) with frame weights (None: 1 / t), two-pass."""
    a = np.asarray(a, dtype=dt)
    b, t, c = a.shape
    w = np.full((b, t), dt(1), dt) if weights is None else np.asarray(weights, dtype=dt).reshape(b, t)
    n = rsum(w, 1, dt)[:, None]
    # the mean about the frame of the largest weight: a chunk of equal frames then has exactly that value for its mean and a variance of
    # exactly 0, as Welford's update has
    a0 = np.take_along_axis(a, np.argmax(w, axis=1)[:, None, None], axis=1)[:, 0]
    mean = a0 + rsum((a - a0[:, None]) * w[:, :, None], 1, dt) / n
    var = rsum(w[:, :, None] * (a - mean[:, None]) ** 2, 1, dt) / n
    return mean, np.sqrt(np.maximum(var, dt(VAR_EPS))), var


def stat_pool_bound(a, d_a, weights=None):
    """Bounds of the pooled mean and std of activations a (float64) known to within d_a per element.

    mean: the kernel's running mean m_k = m_(k-1) + (a_k - m_(k-1)) w_k / n_k takes 4 roundings per step (difference, quotient - v_rcp_f32: 1 ulp,
    counted as 2 -, product, sum).  The sum's rounding u |m_k| is damped by n_k / n afterwards and |m_k| n_k <= sum_(j<=k) w_j |a_j|, so the L
    steps of a chain leave at most L u A, A = sum w |a| / n; the other three act on the difference, within the range R = max a - min a of the
    frames that carry weight, times w_k / n_k, damped alike: 4 u R (one u to spare).  A weighted mean moves by at most the largest input error:
      d mean = u (L A + 4 R) + max d_a
    var: M2 grows by (a_k - m_(k-1)) (a_k - m_k) w_k, factors within R: 4 u R^2 for the roundings of the terms, L u var for the chain,
    2 R e for the errors of the running means and of the inputs, and their square:
      d var = (L + 6) u var + 4 u R^2 + 2 R e + e^2,  e = u (L A + 4 R) + 2 max d_a
    Frames of weight 0 leave the kernel's state as it is (their terms are multiplied by 0): they count in none of A, R, max d_a.
    std = sqrt(max(var, 1e-12)): the larger of the two one-sided moves over [var - d var, var + d var], + 2 u std (division by n, sqrt)."""
    a = f64(a)
    b, t, c = a.shape
    L = pool_chain(t)
    mean, sd, var = stat_pool(a, weights)
    w = np.ones((b, t)) if weights is None else f64(weights).reshape(b, t)
    live = (w > 0)[:, :, None]
    A = (np.abs(a) * w[:, :, None]).sum(axis=1) / w.sum(axis=1)[:, None]
    R = np.where(live, a, -np.inf).max(axis=1) - np.where(live, a, np.inf).min(axis=1)
    da = np.where(live, d_a, 0.0).max(axis=1) if np.ndim(d_a) == 3 else np.zeros((b, c))
    d_mean = U * (L * A + 4 * R) + da
    e = U * (L * A + 4 * R) + 2 * da
    d_var = (L + 6) * U * var + 4 * U * R ** 2 + 2 * R * e + e ** 2
    hi, lo = np.sqrt(np.maximum(var + d_var, VAR_EPS)), np.sqrt(np.maximum(var - d_var, VAR_EPS))
    return d_mean, np.maximum(hi - sd, sd - lo) + 2 * U * sd


def stat_pool_bn(z, b, t, scale, shift, relu, slope, weights=None, dt=np.float64):
    """Pooled statistics of act(z scale + shift) with wpos (the share of the frame weights on frames with a positive activation; all frames
    without an activation) and amax (the chunk's largest activation) per chunk and channel."""
    a = bn_apply(z, scale, shift, relu, slope, dt).reshape(b, t, -1)
    mean, sd, _ = stat_pool(a, weights, dt)
    w = np.full((b, t), dt(1), dt) if weights is None else np.asarray(weights, dtype=dt).reshape(b, t)
    on = (a > 0) if relu else np.ones(a.shape, bool)
    wpos = rsum(w[:, :, None] * on, 1, dt) / rsum(w, 1, dt)[:, None]
    return mean, sd, wpos, a.max(axis=1)


def stat_pool_bn_bound(z, b, t, scale, shift, relu, slope, weights=None):
    """mean, std: stat_pool_bound with d_a = bn_apply_bound.  wpos: the lane sums of the weights (ceil(t / 4) + 2 additions), the sum n of the
    weights, its reciprocal and the product: (ceil(t / 4) + 6) u wpos, plus the weight of every ambiguous frame.  amax: the largest d_a of the chunk."""
    n = z.shape[1]
    a = bn_apply(z, scale, shift, relu, slope).reshape(b, t, n)
    d_a = bn_apply_bound(z, scale, shift, relu, slope).reshape(b, t, n)
    d_mean, d_sd = stat_pool_bound(a, d_a, weights)
    _, _, amb, _ = pre_activation(z, scale, shift)
    w = np.ones((b, t)) if weights is None else f64(weights).reshape(b, t)
    wn = w / w.sum(axis=1, keepdims=True)
    _, _, wpos, _ = stat_pool_bn(z, b, t, scale, shift, relu, slope, weights)
    d_wpos = (cdiv(t, 4) + 6) * U * wpos + ((wn[:, :, None] * amb.reshape(b, t, n)).sum(axis=1) if relu else 0.0)
    return d_mean, d_sd, d_wpos, d_a.max(axis=1)


def stat_pool_backward(x, out, dout, dt=np.float64):
    """dx = dmean / t + (dstd / std / t) (x - mean), the std term 0 where the float32 std sits at the clamp."""
    x = np.asarray(x, dtype=dt)
    b, t, c = x.shape
    o, g = np.asarray(out, dtype=dt), np.asarray(dout, dtype=dt)
    inv_t = dt(1) / dt(t)
    k = np.where(f32(out)[:, c:] <= np.sqrt(np.float32(1e-12)), dt(0), g[:, c:] / o[:, c:] * inv_t)
    return g[:, None, :c] * inv_t + k[:, None] * (x - o[:, None, :c])


def stat_pool_backward_bound(x, out, dout):
    """1 / t, two products, a division, the difference, the sum: 6 u (|dmean / t| + |k (x - mean)|)."""
    x = f64(x)
    b, t, c = x.shape
    o, g = f64(out), f64(dout)
    k = np.where(f32(out)[:, c:] <= np.sqrt(np.float32(1e-12)), 0.0, g[:, c:] / o[:, c:] / t)
    return 6 * U * (np.abs(g[:, None, :c]) / t + np.abs(k[:, None] * (x - o[:, None, :c])))


# ------------------------------------------------------------------ l2_scaling
L2_EPS32 = np.float32(1e-12)


def l2_chain(n):
    """A lane adds its ceil(n / 64) squares in order, then six butterfly steps across the wave."""
    return cdiv(n, 64) + 6


def l2_scaling(x, factor, dt=np.float64):
    x = np.asarray(x, dtype=dt)
    ss = (x * x).sum(axis=1, dtype=dt, keepdims=True)
    inv = dt(1) / np.sqrt(np.maximum(ss, dt(L2_EPS32))) * dt(np.float32(factor))
    return x * inv, ss, inv


def l2_rel_inv(n):
    """Relative error of inv = rsqrt(max(ss, eps)) factor: half of that of ss ((L + 1) u: a square rounds once), rsqrt within 2 ulp (4 u), the product."""
    return (0.5 * (l2_chain(n) + 1) + 5) * U


def l2_scaling_bound(x, factor):
    y, _, _ = l2_scaling(x, factor)
    return (l2_rel_inv(x.shape[1]) + U) * np.abs(y)


def l2_scaling_backward(x, dy, factor, live=None, dt=np.float64):
    """dx = dy inv - x (inv / ss) (x . dy) where ss >= eps (tf.maximum hands the gradient to ss on a tie), dy inv where the clamp holds.
    live: the rows whose float32 sum of squares is known to sit exactly on the threshold are given explicitly."""
    x, dy = np.asarray(x, dtype=dt), np.asarray(dy, dtype=dt)
    _, ss, inv = l2_scaling(x, factor, dt)
    if live is None:
        live = ss >= dt(L2_EPS32)
    dot = (x * dy).sum(axis=1, dtype=dt, keepdims=True)
    k = np.where(live, inv / np.where(ss > 0, ss, dt(1)) * dot, dt(0))
    return dy * inv - x * k


def l2_scaling_backward_bound(x, dy, factor, live=None):
    """k = inv / ss dot: d k = |inv / ss| (L + 1) u sum|x dy| + |k| (rel(inv) + (L + 1) u + 2 u);  dx: |dy inv| (rel(inv) + u) + |x| d k + u |x k|, and the
    subtraction: u (|dy inv| + |x k|)."""
    x, dy = f64(x), f64(dy)
    n = x.shape[1]
    _, ss, inv = l2_scaling(x, factor)
    if live is None:
        live = ss >= float(L2_EPS32)
    L = l2_chain(n)
    safe = np.where(ss > 0, ss, 1.0)
    dot = (x * dy).sum(axis=1, keepdims=True)
    k = np.where(live, inv / safe * dot, 0.0)
    d_k = np.where(live, np.abs(inv / safe) * (L + 1) * U * np.abs(x * dy).sum(axis=1, keepdims=True) + np.abs(k) * (l2_rel_inv(n) + (L + 3) * U), 0.0)
    return np.abs(dy * inv) * (l2_rel_inv(n) + 2 * U) + np.abs(x) * d_k + 2 * U * np.abs(x * k)


def l2_threshold_row(n):
    """A float32 row of n >= 2 elements whose sum of squares is, in float32 and whatever the order of the additions, exactly the clamp value
    float32(1e-12): x0 = 2^-20 (its square 2^-40 is exact), x1 chosen so that fl(2^-40 + fl(x1^2)) is the clamp value, zeros elsewhere."""
    row = np.zeros(n, np.float32)
    row[0] = np.float32(2.0 ** -20)
    rest = np.float32(L2_EPS32 - row[0] * row[0])
    x1 = np.float32(np.sqrt(np.float64(rest)))
    for _ in range(64):
        s = np.float32(row[0] * row[0] + np.float32(x1 * x1))
        if s == L2_EPS32:
            row[1] = x1
            return row
        x1 = np.nextafter(x1, np.float32(1.0 if s < L2_EPS32 else 0.0))
    raise AssertionError("no float32 x1 puts the sum of squares on the threshold")


# ------------------------------------------------------------------ the same interface as the GPU backend, in plain float32 NumPy
class NumpyOps(object):
    """Every op of the rows as a plain float32 NumPy evaluation of the formulas above (NumPy's own summation order): what the bounds are
    held against before a kernel runs."""
    name = "numpy-float32"
    dt = np.float32

    def col_stats(self, z, layout=None, want_form=None):
        return f32(col_stats(z, self.dt))

    def bn_finalize(self, part, rows, gamma, beta, eps, momentum, unbiased, mm, mv, with_range=False, relu=True, slope=None):
        out = {k: f32(v) for k, v in bn_finalize(part, rows, gamma, beta, eps, momentum, unbiased, mm, mv, self.dt).items()}
        if with_range:
            out["amax"] = output_range_amax(out["zmin"], out["zmax"], out["scale"], out["shift"], relu, slope if relu else None)
        return out

    def bn_output_range(self, part, rows, scale, shift, relu, slope=None):
        zmin, zmax = f32(part[2].min(axis=0)), f32(part[3].max(axis=0))
        return zmin, zmax, output_range_amax(zmin, zmax, scale, shift, relu, slope if relu else None)

    def bn_inference_scale(self, gamma, beta, mm, mv, eps):
        return tuple(f32(v) for v in bn_inference_scale(gamma, beta, mm, mv, eps, self.dt))

    def bn_apply(self, z, scale, shift, relu, slope=None, ldz=None, lda=None):
        return f32(bn_apply(z, scale, shift, relu, slope, self.dt))

    def bn_backward(self, z, gamma, mean, invstd, scale, shift, relu, slope=None, want_dalpha=False, da=None, segs=None, t=None, pad=0,
                    pooled=None, wpos=None):
        rows = z.shape[0]
        red = bn_backward(z, gamma, mean, invstd, scale, shift, relu, slope, 0, da=da, pooled=pooled, dt=self.dt)
        if wpos is not None:
            dbeta, dgamma, _, _ = closed_form(pooled[0], pooled[1], wpos, gamma, mean, invstd, scale, shift, rows, self.dt)
        else:
            dbeta, dgamma = red["dbeta"], red["dgamma"]
        dz, _ = bn_backward_dz(red, z, gamma, mean, invstd, dbeta, dgamma, self.dt)
        if pooled is None:
            dz = pad_rows(dz, segs, t, pad)
        g_is = np.asarray(gamma, self.dt) * np.asarray(invstd, self.dt)
        c1 = dbeta / self.dt(rows)
        out = dict(dz=f32(dz), dgamma=f32(dgamma), dbeta=f32(dbeta), dbias=f32(g_is * (dbeta - c1 * self.dt(rows))))
        if want_dalpha:
            out["dalpha"] = f32(red["dalpha"])
        return out

    def stat_pool_forward(self, x):
        mean, sd, _ = stat_pool(x, None, self.dt)
        return f32(np.concatenate([mean, sd], axis=1))

    def stat_pool_forward_bn(self, z, b, t, scale, shift, relu, slope=None, weights=None, aux=True):
        mean, sd, wpos, amax = stat_pool_bn(z, b, t, scale, shift, relu, slope, weights, self.dt)
        out = f32(np.concatenate([mean, sd], axis=1))
        return (out, f32(wpos), f32(amax)) if aux else out

    def stat_pool_backward(self, x, out, dout):
        return f32(stat_pool_backward(x, out, dout, self.dt))

    def l2_scaling_forward(self, x, factor):
        return f32(l2_scaling(x, factor, self.dt)[0])

    def l2_scaling_backward(self, x, dy, factor):
        return f32(l2_scaling_backward(x, dy, factor, dt=self.dt))
