"""NumPy restatement of GhostVLAD / NetVLAD pooling (reference model/pooling.py:195-277; kernels in csrc/xv_vlad.hip), forward and backward,
with the rounding bound of each kernel's output - what tests/test_gpu_vlad.py compares the kernels with, and the pooling that
tests/test_gpu_vlad_engine.py puts into the float64 oracle of the whole step.

As in tests/attention_ref.py: every formula takes a dtype, float64 is the reference and float32 the plain NumPy evaluation that
tests/test_vlad_ref.py holds against the same bounds before a kernel runs; u = 2^-24; a sum of terms t_i with a longest addition chain of L
and c roundings per term is within (L + c) u sum|t_i| of the exact sum; nothing is relative to a tensor's largest entry.

    A_t = softmax(x_t W + b) over K + G clusters          n_k = sum_t A_tk           R_k = sum_t A_tk (x_t - c_k)      (k < K)
    V_k = R_k rsqrt(max(|R_k|^2, eps))                    out = [V_0 .. V_{K-1}] (final_l2_norm: out rsqrt(max(|out|^2, eps)))
eps = float32(1e-12) is tf.nn.l2_normalize's; the reference's NumPy statement (model/test_utils.py:421-436) divides without it.

Where no bound is derived - the normalisation backward, whose terms cancel (the gradient is projected off R) and whose branch at
|R|^2 = eps is a step - `close_to_f32_eval` compares with the float32 NumPy evaluation of the same formulas instead: the kernel may be 8 times as
far from float64 as that evaluation is (the order of the additions differs), per chunk, and never has to be closer than 8 roundings of the
chunk's largest entry (an evaluation that happens to be exact in float32 sets no zero tolerance).

Transcendental functions: HIP's table gives 1 ulp for expf and rsqrtf; as in attention_ref the same allowance again covers NumPy's:
EXP_REL = RSQRT_REL = 2 * 1 * 2 u."""
import numpy as np

U = 2.0 ** -24
EXP_REL = 2 * 1 * 2 * U
RSQRT_REL = 2 * 1 * 2 * U
FLT_MIN = 2.0 ** -126
EPS32 = np.float32(1e-12)
GROUP = 8          # clusters per pass of the pooling kernels (VL_G)


def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def f64(a):
    return np.asarray(a, dtype=np.float64)


def cdiv(a, b):
    return -(-a // b)


def row_chain(c):
    """A wave's sum over c columns: (p0 + p1) + (p2 + p3) per quad (2), a lane's ceil(c / 4 / 64) quads in order, six butterfly steps."""
    return cdiv(cdiv(c, 4), 64) + 2 + 6


# ------------------------------------------------------------------ assignment softmax (one wave per frame: six butterfly steps)
def softmax(logits, dt=np.float64):
    s = np.asarray(logits, dtype=dt)
    e = np.exp(s - s.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True, dtype=dt)


def softmax_bound(logits):
    """attention_ref.softmax_bound with the chain of a single wave (L = 6)."""
    s = f64(logits)
    d = np.abs(s - s.max(axis=1, keepdims=True))
    w = softmax(s)
    eps = U * d + EXP_REL
    return w * (eps + (6 + 1) * U + (w * eps).sum(axis=1, keepdims=True)) * (1 + 1e-3) + FLT_MIN


def softmax_backward(a, da, dt=np.float64):
    a, da = np.asarray(a, dtype=dt), np.asarray(da, dtype=dt)
    return a * (da - (a * da).sum(axis=1, keepdims=True, dtype=dt))


def softmax_backward_bound(a, da):
    """attention_ref.softmax_backward_bound, L = 6."""
    a, da = f64(a), f64(da)
    z = (a * da).sum(axis=1, keepdims=True)
    dz = (6 + 1) * U * np.abs(a * da).sum(axis=1, keepdims=True)
    return np.abs(a) * (dz + U * (np.abs(da) + np.abs(z))) + U * np.abs(a * (da - z)) + (a.shape[1] + 2) * FLT_MIN


# ------------------------------------------------------------------ pooling
def valid_frames(t, frames, shrink):
    """Rows chunk i pools: all t, or max(1, min(t, frames[i] - shrink)) (batched extraction)."""
    return None if frames is None else np.maximum(1, np.minimum(t, np.asarray(frames, np.int64) - int(shrink)))


def pool_forward(x, a, cen, k, frames=None, shrink=0, dt=np.float64):
    """x [b, t, c], a [b*t, kg], cen [kg, c] -> R [b, k, c], n [b, k]"""
    x, cen = np.asarray(x, dtype=dt), np.asarray(cen, dtype=dt)
    b, t, c = x.shape
    a3 = np.asarray(a, dtype=dt).reshape(b, t, -1)[:, :, :k].copy()
    tv = valid_frames(t, frames, shrink)
    if tv is not None:
        for i in range(b):
            a3[i, tv[i]:] = 0
    r = np.empty((b, k, c), dt)
    for j in range(k):
        r[:, j] = (a3[:, :, j:j + 1] * (x - cen[j])).sum(axis=1, dtype=dt)
    return r, a3.sum(axis=1, dtype=dt)


def pool_forward_bound(x, a, cen, k, frames=None, shrink=0, chain=None):
    """A frame lane adds its ceil(t / 4) frames in order, then three merges: L = ceil(t / 4) + 3.  A term a (x - c) rounds the difference and
    (fused with the addition) nothing more: c = 1, one to spare.  n: the same chain on the weights themselves.
    chain: the longest addition chain of another evaluation of the same sums (NumPy's float32 one: at most t - 1 in any order, and its
    product rounds on its own - inside the one to spare)."""
    x, cen = f64(x), f64(cen)
    b, t, c = x.shape
    a3 = np.abs(f64(a).reshape(b, t, -1)[:, :, :k]).copy()
    tv = valid_frames(t, frames, shrink)
    if tv is not None:
        for i in range(b):
            a3[i, tv[i]:] = 0
    L = cdiv(t, 4) + 3 if chain is None else int(chain)
    mag = np.empty((b, k, c))
    for j in range(k):
        mag[:, j] = (a3[:, :, j:j + 1] * np.abs(x - cen[j])).sum(axis=1)
    return (L + 2) * U * mag + t * FLT_MIN, L * U * a3.sum(axis=1) + t * FLT_MIN      # (+ a term under FLT_MIN may be flushed to zero)


def pool_backward(x, a, cen, dr, dt=np.float64):
    """-> dA [b*t, kg] ((x - c_k) . dR_k, 0 for the ghosts), dx [b, t, c] (sum_k A dR_k)"""
    x, cen, dr = np.asarray(x, dtype=dt), np.asarray(cen, dtype=dt), np.asarray(dr, dtype=dt)
    b, t, c = x.shape
    k, kg = dr.shape[1], cen.shape[0]
    a3 = np.asarray(a, dtype=dt).reshape(b, t, kg)
    da = np.zeros((b, t, kg), dt)
    dx = np.zeros((b, t, c), dt)
    for j in range(k):
        da[:, :, j] = ((x - cen[j]) * dr[:, None, j]).sum(axis=2, dtype=dt)
        dx += a3[:, :, j:j + 1] * dr[:, None, j]
    return da.reshape(b * t, kg), dx


def pool_backward_bound(x, a, cen, dr, chain=None):
    """dA: a wave's row sum of (x - c) dR - the difference and the product round: (row_chain + 2) u sum|.|.  dx: the clusters in order, fused
    multiply-adds: (K + 1) u sum_k |A dR|; a further group of clusters adds to the float32 it stored - covered by the + 1 per group."""
    x, cen, dr = f64(x), f64(cen), f64(dr)
    b, t, c = x.shape
    k, kg = dr.shape[1], cen.shape[0]
    a3 = np.abs(f64(a).reshape(b, t, kg))
    bda = np.zeros((b, t, kg))
    mdx = np.zeros((b, t, c))
    for j in range(k):
        bda[:, :, j] = (np.abs(x - cen[j]) * np.abs(dr[:, None, j])).sum(axis=2)
        mdx += a3[:, :, j:j + 1] * np.abs(dr[:, None, j])
    L = row_chain(c) if chain is None else int(chain)      # (chain: another evaluation's longest chain over the c columns, see pool_forward_bound)
    return (L + 2) * U * bda.reshape(b * t, kg) + c * FLT_MIN, (k + 1 + cdiv(k, GROUP)) * U * mdx + k * FLT_MIN


def centers_backward(n, dr, cen, l2, dt=np.float64):
    """dc [kg, c] = l2 c - sum_b n dR for k < K"""
    n, dr, cen = np.asarray(n, dtype=dt), np.asarray(dr, dtype=dt), np.asarray(cen, dtype=dt)
    dc = cen * dt(np.float32(l2))
    dc[:dr.shape[1]] -= (n[:, :, None] * dr).sum(axis=0, dtype=dt)
    return dc


def centers_backward_bound(n, dr, cen, l2, chain=None):
    """A chunk lane adds chunks lane, lane + 16, ... in order (fused), the 16 lanes are added in order (a lane without a chunk adds an exact
    zero): L = ceil(b / 16) + min(b, 16); the regulariser's product and the difference: (L + 2) u (sum_b |n dR| + |l2 c|).
    chain: another evaluation's longest chain over the b chunks (see pool_forward_bound)."""
    n, dr, cen = f64(n), f64(dr), f64(cen)
    mag = np.abs(cen) * abs(float(np.float32(l2)))
    mag[:dr.shape[1]] += (np.abs(n)[:, :, None] * np.abs(dr)).sum(axis=0)
    b = dr.shape[0]
    L = cdiv(b, 16) + min(b, 16) if chain is None else int(chain)
    return (L + 2) * U * mag + (b + 1) * FLT_MIN


# ------------------------------------------------------------------ normalisations
def _inv(ss, dt):
    return dt(1) / np.sqrt(np.maximum(ss, dt(EPS32)))


def normalize_forward(r, final, dt=np.float64):
    """r [b, k, c] -> [b, k c]"""
    r = np.asarray(r, dtype=dt)
    b, k, c = r.shape
    ss = (r * r).sum(axis=2, dtype=dt)
    inv = _inv(ss, dt)
    v = r * inv[:, :, None]
    if final:
        s = (ss * inv * inv).sum(axis=1, dtype=dt)
        v = v * _inv(s, dt)[:, None, None]
    return v.reshape(b, k * c)


def normalize_forward_bound(r, final):
    """|R_k|^2: (row_chain + 1) u relative (all terms positive); its rsqrt halves that and has its allowance; the product rounds once.  final:
    s = sum_k |R_k|^2 inv_k^2 - per term the sum's error, twice the rsqrt's, two products - over K additions; its rsqrt; two more products."""
    r = f64(r)
    b, k, c = r.shape
    rel_ss = (row_chain(c) + 1) * U
    rel_inv = 0.5 * rel_ss + RSQRT_REL
    rel = rel_inv + U
    if final:
        rel_s = rel_ss + 2 * rel_inv + 2 * U + k * U
        rel = rel + 0.5 * rel_s + RSQRT_REL + 2 * U
    return np.abs(normalize_forward(r, final)) * rel * (1 + 1e-3) + FLT_MIN


def normalize_backward(r, dout, final, dt=np.float64):
    """d R.  y = V f: dV = f dy - [s >= eps] f^3 (V . dy) V;  V_k = R_k inv_k: dR = inv dV - [|R|^2 >= eps] inv^3 (R . dV) R.  A clamped
    norm is the constant 1 / sqrt(eps) (tf.maximum passes no gradient to the smaller argument)."""
    r = np.asarray(r, dtype=dt)
    b, k, c = r.shape
    g = np.asarray(dout, dtype=dt).reshape(b, k, c)
    eps = dt(EPS32)
    ss = (r * r).sum(axis=2, dtype=dt)
    inv = _inv(ss, dt)
    if final:
        v = r * inv[:, :, None]
        s = (ss * inv * inv).sum(axis=1, dtype=dt)
        f = _inv(s, dt)
        d = (v * g).sum(axis=(1, 2), dtype=dt)
        cf = np.where(s >= eps, f * f * f * d, dt(0))
        g = f[:, None, None] * g - cf[:, None, None] * v
    q = (r * g).sum(axis=2, dtype=dt)
    ck = np.where(ss >= eps, inv * inv * inv * q, dt(0))
    return inv[:, :, None] * g - ck[:, :, None] * r


def close_to_f32_eval(got, ref64, eval32):
    """(ok, worst ratio, per-chunk figures): per chunk (first axis) max|got - ref64| <= 8 max(max|eval32 - ref64|, u max|ref64|)."""
    got, ref64, eval32 = f64(got), f64(ref64), f64(eval32)
    ax = tuple(range(1, ref64.ndim))
    err = np.abs(got - ref64).max(axis=ax)
    own = np.abs(eval32 - ref64).max(axis=ax)
    tol = 8 * np.maximum(own, U * np.abs(ref64).max(axis=ax))
    ratio = err / np.where(tol > 0, tol, 1.0)
    return bool(np.all(err <= tol)), float(ratio.max()), (err, own, tol)


# ------------------------------------------------------------------ the whole layer (float64 oracle of the engine tests)
def vlad_forward(x, w, bias, cen, k, final, frames=None, shrink=0, dt=np.float64):
    """x [b, t, c] -> (out [b, k c], cache)"""
    x = np.asarray(x, dtype=dt)
    b, t, c = x.shape
    logits = x.reshape(b * t, c) @ np.asarray(w, dtype=dt) + np.asarray(bias, dtype=dt)
    a = softmax(logits, dt)
    r, n = pool_forward(x, a, cen, k, frames, shrink, dt)
    out = normalize_forward(r, final, dt)
    return out, dict(x=x, w=np.asarray(w, dtype=dt), cen=np.asarray(cen, dtype=dt), a=a, r=r, n=n, k=k, final=final, logits=logits)


def vlad_backward(dout, cache, l2=0.0, dt=np.float64):
    """-> dx [b, t, c], dW [c, kg], dbias [kg], dcen [kg, c] (dW and dcen with the regulariser's l2 W, l2 c)"""
    x, w, cen, a, r, n = (cache[key] for key in ("x", "w", "cen", "a", "r", "n"))
    b, t, c = x.shape
    dr = normalize_backward(r, dout, cache["final"], dt)
    dcen = centers_backward(n, dr, cen, l2, dt)
    da, dx = pool_backward(x, a, cen, dr, dt)
    dl = softmax_backward(a, da, dt)
    x2 = x.reshape(b * t, c)
    dw = x2.T @ dl + dt(np.float32(l2)) * w
    dx = dx + (dl @ w.T).reshape(b, t, c)
    return dx, dw, dl.sum(axis=0, dtype=dt), dcen


# ------------------------------------------------------------------ inputs
def make_case(rs, b, t, c, k, g, hostile=False):
    """Post-ReLU-like values, an assignment layer and centres of the reference's initialisers' scale.  hostile: the four chunks of the
    reference's self-test (model/pooling.py:478-510): x 1e-8, all zero, x 100, the constant 100."""
    kg = k + g
    x = np.maximum(rs.randn(b, t, c), 0) + 0.1 * rs.rand(b, t, c)
    if hostile:
        assert b >= 4
        x[0] *= 1e-8
        x[1] = 0.0
        x[2] *= 100.0
        x[3] = 100.0
    lim = np.sqrt(6.0 / (c + kg))
    w = rs.uniform(-lim, lim, size=(c, kg))
    bias = 0.1 * rs.randn(kg)
    cen = rs.uniform(-lim, lim, size=(kg, c))
    return f32(x), f32(w), f32(bias), f32(cen)
