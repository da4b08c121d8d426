"""NumPy restatement of the segment-level GEMM kernel (csrc/xv_skinny.hip: the plain epilogue, the training-mode BatchNorm epilogue and the
BatchNorm-backward epilogue) with the rounding bound of each output, what tests/test_gpu_segment_forms.py compares the kernel with.

As in tests/bn_pool_ref.py: every formula takes a dtype, float64 is the reference and float32 the plain NumPy evaluation that
tests/test_segment_ref.py holds against the same bounds before the kernel runs (class NumpyOps); u = 2^-24; a sum of terms t_i with a longest
addition chain of L and c roundings per term is within (L + c) u sum|t_i| of the exact sum; bounds are per element or per channel, never
relative to a tensor's largest entry.  Helpers (pre_activation, act, bn_backward, bn_backward_dz, ...) are those of tests/bn_pool_ref.py."""
import numpy as np

import bn_pool_ref as R
from bn_pool_ref import U, f32, f64

# a column's reduction over the rows (sk_col_sum): a lane's 16 accumulator rows in order, the two lane halves, (w0 + w1) + (w2 + w3)
COL_L = 16 + 1 + 2


# ------------------------------------------------------------------ input families
def make_operands(rs, m, n, k, family="base"):
    """a [m][k] = randn, bt [n][k] = randn / sqrt(k), bias [n] = randn (the scaling of tests/test_gpu_ops.py); heterogeneous: output column c (a
    row of bt, an entry of bias) carries 10^(c mod 7 - 3)."""
    a, bt, bias = rs.randn(m, k), rs.randn(n, k) / np.sqrt(k), rs.randn(n)
    if family == "hetero":
        cs = R.channel_scale(n)
        bt, bias = bt * cs[:, None], bias * cs
    return f32(a), f32(bt), f32(bias)


def make_row_term(rs, m, n, family="base"):
    """coef, norm, X of the rank-one row term: norm[0] = 0 (the guarded division), one negative coefficient at least."""
    coef, norm, x = rs.randn(m), np.abs(rs.randn(m)) + 0.1, rs.randn(m, n)
    norm[0] = 0.0
    coef[m - 1] = -abs(coef[m - 1]) - 0.1
    if family == "hetero":
        x = x * R.channel_scale(n)
    return f32(coef), f32(norm), f32(x)


# ------------------------------------------------------------------ GEMM with the plain epilogue
def row_factor(row_term, dt=np.float64):
    coef, norm, x = row_term
    coef, norm = np.asarray(coef, dtype=dt), np.asarray(norm, dtype=dt)
    return np.where(norm > 0, coef / np.where(norm > 0, norm, dt(1)), dt(0))


def gemm(a, bt, bias=None, row_term=None, dt=np.float64):
    """C[m][n] = sum_k a[m][k] bt[n][k] (+ (norm[m] > 0 ? coef[m] / norm[m] : 0) X[m][n]) (+ bias[n])"""
    c = np.asarray(a, dtype=dt) @ np.asarray(bt, dtype=dt).T
    if row_term is not None:
        c = c + row_factor(row_term, dt)[:, None] * np.asarray(row_term[2], dtype=dt)
    if bias is not None:
        c = c + np.asarray(bias, dtype=dt)
    return c


def gemm_bound(a, bt, bias, row_term, k_chunk, splits):
    """The MFMA chain adds one k at a time over a split's k_chunk (over K where K is shorter than the 32-aligned chunk: the zero page adds
    nothing), the slabs are added in split order: L = min(k_chunk, K) + splits, a product rounds once: (L + 1) u S, S = sum_k |a b|.
    The row term t = fl(fl(coef / norm) X) carries two roundings and its addition a third: 3 u |t| + u S; the bias's addition u (S + |t| + |bias|).  Together (L + 3) u S + 4 u |t| + u |bias|."""
    S = np.abs(f64(a)) @ np.abs(f64(bt)).T
    t = 0.0 if row_term is None else np.abs(row_factor(row_term)[:, None] * f64(row_term[2]))
    b = 0.0 if bias is None else np.abs(f64(bias))
    return (min(k_chunk, np.shape(a)[1]) + splits + 3) * U * S + 4 * U * t + U * b


# ------------------------------------------------------------------ BatchNorm forward epilogue
def bn_forward(z, gamma, beta, eps, momentum, unbiased, mm, mv, dt=np.float64):
    """Statistics of the m rows of z as the epilogue forms them: mean, two-pass biased variance, invstd = 1 / sqrt(var + eps), scale = gamma
    invstd, shift = beta - mean scale; moving = old momentum + new (1 - momentum) with the float32 (1 - momentum), the variance with Bessel's
    factor when unbiased and m > 1."""
    z = np.asarray(z, dtype=dt)
    m = z.shape[0]
    mean = R.rsum(z, 0, dt) / dt(m)
    var = R.rsum((z - mean) ** 2, 0, dt) / dt(m)
    invstd = dt(1) / np.sqrt(var + dt(np.float32(eps)))
    scale = np.asarray(gamma, dtype=dt) * invstd
    out = dict(mean=mean, invstd=invstd, scale=scale, shift=np.asarray(beta, dtype=dt) - mean * scale)
    if mm is not None:
        mom, om = dt(np.float32(momentum)), dt(np.float32(1) - np.float32(momentum))
        v = var * (dt(m) / dt(m - 1)) if (unbiased and m > 1) else var
        out["moving_mean"] = np.asarray(mm, dtype=dt) * mom + mean * om
        out["moving_var"] = np.asarray(mv, dtype=dt) * mom + v * om
    return out


def bn_forward_bound(z, gamma, beta, eps, momentum, unbiased, mm, mv):
    """On the float32 z the launch returned (the registers the kernel normalises are the values it wrote).
    mean = fl(sum / m): d mean = (L u sum|z|) / m + u |mean|, L = COL_L.
    var: the squares are centred on the float32 mean m^; sum (z - m^)^2 = Q + m (mean - m^)^2 exactly (the cross term vanishes about the true
      mean) and a term carries 3 roundings: d var = ((L + 3) u Q + m d mean^2) / m + u var.
    invstd: 1/2 invstd^3 (d var + u (var + eps)) + 3 u invstd.   scale: |gamma| d invstd + u |scale|.
    shift: |scale| d mean + |mean| d scale + 2 u (|beta| + |mean scale|).
    moving: (1 - momentum) d new + 2 u (|old momentum| + |new (1 - momentum)|); Bessel's factor adds 2 u v."""
    z, gamma, beta = f64(z), f64(gamma), f64(beta)
    m = z.shape[0]
    eps = float(np.float32(eps))
    ref = bn_forward(z, gamma, beta, eps, momentum, unbiased, mm, mv)
    mean = ref["mean"]
    var = ((z - mean) ** 2).mean(axis=0)
    d_mean = COL_L * U * np.abs(z).sum(axis=0) / m + U * np.abs(mean)
    d_var = ((COL_L + 3) * U * var * m * (1 + 1e-3) + m * d_mean ** 2) / m + U * var
    d_invstd = 0.5 * ref["invstd"] ** 3 * (d_var + U * (var + eps)) * (1 + 1e-3) + 3 * U * ref["invstd"]
    d_scale = np.abs(gamma) * d_invstd + U * np.abs(ref["scale"])
    d_shift = np.abs(ref["scale"]) * d_mean + np.abs(mean) * d_scale + 2 * U * (np.abs(beta) + np.abs(mean * ref["scale"]))
    bound = dict(mean=d_mean, invstd=d_invstd, scale=d_scale, shift=d_shift)
    if mm is not None:
        mom, om = float(np.float32(momentum)), float(np.float32(1) - np.float32(momentum))
        unb = unbiased and m > 1
        v = var * m / (m - 1.0) if unb else var
        d_v = d_var * (m / (m - 1.0) if unb else 1.0) + (2 * U * v if unb else 0.0)
        bound["moving_mean"] = om * d_mean + 2 * U * (np.abs(f64(mm) * mom) + np.abs(mean * om))
        bound["moving_var"] = om * d_v + 2 * U * (np.abs(f64(mv) * mom) + np.abs(v * om))
    return ref, bound


def handed_statistics(z, gamma, beta, eps):
    """mean, invstd, scale, shift as float32 vectors to hand to the backward epilogue (any values serve: the kernel takes them as given)."""
    s = bn_forward(z, gamma, beta, eps, 0.0, False, None, None)
    mean, invstd = f32(s["mean"]), f32(s["invstd"])
    scale = f32(f64(gamma) * f64(invstd))
    return mean, invstd, scale, f32(f64(beta) - f64(mean) * f64(scale))


# ------------------------------------------------------------------ BatchNorm backward epilogue
def bn_backward(da, E, z, gamma, mean, invstd, scale, shift, relu, slope):
    """The reductions of the epilogue from d a in float64 (never written: the reference forms it from the operands) known to within E per
    element (gemm_bound), and their bounds.  R.bn_backward supplies dd, xhat, dbeta, dgamma, dalpha, the ambiguous mask and the bounds of the
    reductions themselves (L = COL_L; a term of dbeta 1 rounding, of dgamma 4, of dalpha 1 plus the error of y); the error of d a adds
      dbeta: sum_m E s,   dgamma: sum_m E s |xhat|,   dalpha: sum_m E |min(y, 0)|      (s = max(1, |slope|): what the mask can stretch it by)."""
    red = R.bn_backward(z, gamma, mean, invstd, scale, shift, relu, slope, COL_L, da=da)
    n = z.shape[1]
    Es = E * R.slope_mag(relu, slope, n)
    red["E_dd"] = Es
    red["b_dbeta"] = red["b_dbeta"] + Es.sum(axis=0)
    red["b_dgamma"] = red["b_dgamma"] + (Es * np.abs(red["xhat"])).sum(axis=0)
    if "b_dalpha" in red:
        red["b_dalpha"] = red["b_dalpha"] + (E * np.abs(np.minimum(red["y"], 0))).sum(axis=0)
    return red


def bn_backward_dz(red, z, gamma, mean, invstd, dbeta, dgamma):
    """dz = gamma invstd (dd - c1 - xhat c2) on the backend's own reductions (their rows check them): R.bn_backward_dz's element-wise bound plus
    |gamma invstd| E s for the error of d a."""
    dz, bound = R.bn_backward_dz(red, z, gamma, mean, invstd, dbeta, dgamma)
    return dz, bound + np.abs(f64(gamma) * f64(invstd)) * red["E_dd"]


def dbias_bound(red, gamma, invstd):
    """dbias = gamma invstd (s1 - fl(fl(s1 / m) m)): zero up to 4 u |gamma invstd| |s1| (two roundings, the subtraction, the product)."""
    return 4 * U * np.abs(f64(gamma) * f64(invstd)) * (np.abs(red["dbeta"]) + red["b_dbeta"]) + 1e-300


# ------------------------------------------------------------------ the same interface as the GPU backend, in plain float32 NumPy
class NumpyOps(object):
    """Plain float32 NumPy (its own summation order; the workspace and the pitches take no part)."""
    name = "numpy-float32"
    dt = np.float32

    def gemm(self, a, bt, bias=None, row_term=None, ws_bytes=None, pitches=None):
        return f32(gemm(a, bt, bias, row_term, self.dt))

    def gemm_queue(self, problems):
        return [self.gemm(*p) for p in problems]

    def bn_forward(self, x, wt, bias, gamma, beta, eps, momentum, unbiased, mm, mv, relu, slope=None, want_a=True, pitches=None):
        z = f32(gemm(x, wt, bias, None, self.dt))
        out = {k: f32(v) for k, v in bn_forward(z, gamma, beta, eps, momentum, unbiased, mm, mv, self.dt).items()}
        out["z"] = z
        if want_a:
            out["a"] = f32(R.bn_apply(z, out["scale"], out["shift"], relu, slope, self.dt))
        return out

    def bn_backward(self, dy, wt, row_term, z, gamma, mean, invstd, scale, shift, relu, slope=None, want_dalpha=False, want_dbias=True, pitches=None):
        m = z.shape[0]
        da = f32(gemm(dy, wt, None, row_term, self.dt))
        red = R.bn_backward(z, gamma, mean, invstd, scale, shift, relu, slope, 0, da=da, dt=self.dt)
        dz, _ = R.bn_backward_dz(red, z, gamma, mean, invstd, red["dbeta"], red["dgamma"], self.dt)
        out = dict(dz=f32(dz), dgamma=f32(red["dgamma"]), dbeta=f32(red["dbeta"]))
        if want_dbias:
            g_is = np.asarray(gamma, self.dt) * np.asarray(invstd, self.dt)
            out["dbias"] = f32(g_is * (red["dbeta"] - red["dbeta"] / self.dt(m) * self.dt(m)))
        if want_dalpha:
            out["dalpha"] = f32(red["dalpha"])
        return out
