"""Op-level Python wrappers over the C-ABI (include/xvector_hip.h, "Op level"): the ops of the training step.

Inputs/outputs are torch CUDA tensors used purely as device buffers; every
function enqueues HIP kernels on torch's current stream.  No arithmetic is done
by torch here.  These are what the per-kernel parity tests call.
The ops of the pipeline stages around the network live in wave_ops.py (those that take PCM), pipeline_ops.py (features, scores, the
back end) and diar_ops.py (the recordings of a diarization call: clustering, VBx, the per-recording PCA) and are re-exported here:
callers write ops.mfcc, ops.score_trials, ops.ahc_cluster ...
"""
import ctypes as C

import torch

try:
    from . import kinds
    from ._host import _f32, _lib, _p, _s, _ws, f32_values, ge2e_rows, pitch4, pitched, workspace
    from .diar_ops import *           # noqa: F401,F403 (its public names are the diarization ops)
    from .pipeline_ops import *       # noqa: F401,F403 (... the pipeline ops)
    from .wave_ops import *           # noqa: F401,F403 (and those of the ops that take PCM)
except ImportError:
    import kinds
    from _host import _f32, _lib, _p, _s, _ws, f32_values, ge2e_rows, pitch4, pitched, workspace
    from diar_ops import *            # noqa: F401,F403
    from pipeline_ops import *        # noqa: F401,F403
    from wave_ops import *            # noqa: F401,F403

TILE_M = 128


def pad_channels(x2d, c_dst):
    rows, c = x2d.shape
    out = _f32((rows, c_dst), x2d)
    _lib.call("xv_pad_channels", _s(), _p(x2d), rows, c, _p(out), c_dst)
    return out


def cm_decode(packed, b, t, d):
    """packed: uint8 device tensor of b chunks (xvector_io.h packed layout) -> [b, t, d] float32 (Kaldi 'CM ' decode on the GPU)."""
    out = torch.empty((b, t, d), dtype=torch.float32, device=packed.device)
    stride = (8 + 8 * d + d * t + 15) // 16 * 16
    _lib.call("xv_cm_decode", _s(), _p(packed), b, t, d, C.c_size_t(stride), _p(out))
    return out


def prep_weight_fwd(kernel, c_pad):
    """kernel: [k, C, O] -> [O, k*c_pad]"""
    k, c, o = kernel.shape
    wt = _f32((o, k * c_pad), kernel)
    _lib.call("xv_prep_weight_fwd", _s(), _p(kernel), k, c, o, _p(wt), c_pad)
    return wt


def prep_weight_dgrad(kernel):
    """kernel: [k, C, O] -> [C, k*O] (taps flipped)"""
    k, c, o = kernel.shape
    wf = _f32((c, k * o), kernel)
    _lib.call("xv_prep_weight_dgrad", _s(), _p(kernel), k, c, o, _p(wf))
    return wf


def affine_forward(x, k, wt, bias, o, with_stats=False, ldz=None):
    """x: [segs, t_in, c_pad] -> z [segs*(t_in-k+1), o] (+ bn_part).  ldz: row pitch of z (>= o; the engine writes 1500 columns on a 1504
    pitch): z is then the [rows, o] view of a [rows, ldz] buffer whose columns o .. ldz-1 the launch does not write."""
    segs, t_in, c_pad = x.shape
    rows = segs * (t_in - k + 1)
    ldz = o if ldz is None else int(ldz)
    z = _f32((rows, ldz), x)
    part = _f32((4, (rows + TILE_M - 1) // TILE_M, o), x) if with_stats else None
    wp, wb = _ws(x)
    _lib.call("xv_affine_forward", _s(), _p(x), segs, t_in, c_pad, k, _p(wt), _p(bias), _p(z), o, ldz, _p(part), wp, wb)
    z = z[:, :o] if ldz != o else z
    return (z, part) if with_stats else z


def backend_affine(x, wt, bias):
    """x [rows, c_pad] (zero padding up to a pitch that is a multiple of 4) times wt [o, c_pad]^T plus bias [o]: the project's fp32 NT GEMM
    (xv_affine_forward, k = 1: a view of a training-step op, hence here).  The caller pads wt / bias with zero rows so that o is a multiple of 4: a GEMM operand."""
    rows, ld = pitched(x, "backend_affine: x")
    if x.shape[1] != ld or wt.shape[1] != ld or not wt.is_contiguous():
        raise ValueError("backend_affine: x must be the whole [rows, pitch] buffer and wt [o, pitch] contiguous")
    return affine_forward(x.view(rows, 1, ld), 1, wt, bias, wt.shape[0])


def affine_dgrad(dz_pad, segs, t_out, o, k, wf, c):
    dx = _f32((segs * (t_out + k - 1), c), dz_pad)
    wp, wb = _ws(dz_pad)
    _lib.call("xv_affine_dgrad", _s(), _p(dz_pad), segs, t_out, o, k, _p(wf), _p(dx), c, wp, wb)
    return dx


def affine_wgrad(x, k, c, dz, dz_seg_pitch, dz_row0, o, kernel, l2_scale):
    segs, t_in, c_pad = x.shape
    dk = _f32((k, c, o), x)
    wp, wb = _ws(x)
    _lib.call("xv_affine_wgrad", _s(), _p(x), segs, t_in, c_pad, k, c, _p(dz), dz_seg_pitch, dz_row0, o, _p(kernel),
              float(l2_scale), _p(dk), wp, wb)
    return dk


def colsum(a):
    rows, n = a.shape
    out = _f32((n,), a)
    wp, wb = _ws(a)
    _lib.call("xv_colsum", _s(), _p(a), rows, n, a.stride(0), _p(out), wp, wb)
    return out


def col_stats(z):
    rows, n = z.shape
    part = _f32((4, (rows + TILE_M - 1) // TILE_M, n), z)
    _lib.call("xv_col_stats", _s(), _p(z), rows, n, z.stride(0), _p(part))
    return part


def bn_finalize(part, rows, gamma, beta, eps, momentum, unbiased, moving_mean, moving_var, with_range=False, relu=True):
    n = gamma.numel()
    mean, invstd, scale, shift = (_f32((n,), gamma) for _ in range(4))
    zmin = _f32((n,), gamma) if with_range else None
    zmax = _f32((n,), gamma) if with_range else None
    amax = torch.zeros(1, dtype=torch.int32, device=gamma.device) if with_range else None
    _lib.call("xv_bn_finalize", _s(), _p(part), rows, n, _p(gamma), _p(beta), float(eps), float(momentum), int(unbiased),
              _p(moving_mean), _p(moving_var), _p(mean), _p(invstd), _p(scale), _p(shift), _p(zmin), _p(zmax), _p(amax), int(relu))
    if with_range:
        return mean, invstd, scale, shift, zmin, zmax, amax.view(torch.float32)
    return mean, invstd, scale, shift


def bn_inference_scale(gamma, beta, moving_mean, moving_var, eps):
    n = gamma.numel()
    scale, shift = _f32((n,), gamma), _f32((n,), gamma)
    _lib.call("xv_bn_inference_scale", _s(), n, _p(gamma), _p(beta), _p(moving_mean), _p(moving_var), float(eps), _p(scale), _p(shift))
    return scale, shift


def bn_output_range(part, rows, scale, shift, relu=True):
    """Per-channel range of z from the min / max planes of `part` (col_stats layout) and the largest |relu?(z*scale+shift)| over the batch
    for the given scale / shift (the activation context applies): -> zmin, zmax [n], amax [1]."""
    n = scale.numel()
    zmin, zmax = _f32((n,), scale), _f32((n,), scale)
    amax = torch.zeros(1, dtype=torch.int32, device=scale.device)
    _lib.call("xv_bn_output_range", _s(), _p(part), rows, n, _p(scale), _p(shift), int(relu), _p(zmin), _p(zmax), _p(amax))
    return zmin, zmax, amax.view(torch.float32)


def bn_apply(z, scale, shift, relu, ldz=None, lda=None, out=None):
    """a = relu?(z*scale+shift).  ldz: floats per row of z (default: z's own row stride); lda: floats per row of the result (default n) -
    the result is then the [rows, n] view of a [rows, lda] buffer (`out`, or a new one)."""
    rows, n = z.shape
    ldz = z.stride(0) if ldz is None else int(ldz)
    lda = n if lda is None else int(lda)
    buf = _f32((rows, lda), z) if out is None else out
    if buf.shape != (rows, lda) or not buf.is_contiguous():
        raise ValueError("bn_apply: out must be a contiguous [rows, lda] buffer")
    _lib.call("xv_bn_apply", _s(), _p(z), rows, n, ldz, _p(scale), _p(shift), int(relu), _p(buf), lda)
    return buf[:, :n]


def bn_relu_backward(da, z, segs, t, gamma, mean, invstd, scale, shift, relu, pad, with_dbias=False):
    n = z.shape[1]
    dz = _f32((segs * (t + 2 * pad), n), z)
    dgamma, dbeta = _f32((n,), z), _f32((n,), z)
    dbias = _f32((n,), z) if with_dbias else None
    wp, wb = _ws(z)
    _lib.call("xv_bn_relu_backward", _s(), _p(da), _p(z), segs, t, n, _p(gamma), _p(mean), _p(invstd), _p(scale), _p(shift),
              int(relu), int(pad), _p(dz), _p(dgamma), _p(dbeta), _p(dbias), wp, wb)
    return (dz, dgamma, dbeta, dbias) if with_dbias else (dz, dgamma, dbeta)


class activation:
    """`with ops.activation(slope, dalpha=None):` - the op-level calls inside take y > 0 ? y : slope[c] * y (prelu / lrelu,
    tdnn.py:24-30) wherever their `relu` flag is set, through the ABI's xv_set_activation; plain ReLU again on exit."""

    def __init__(self, slope, dalpha=None):
        self.slope, self.dalpha = slope, dalpha

    def __enter__(self):
        _lib.call("xv_set_activation", _p(self.slope), _p(self.dalpha))
        return self

    def __exit__(self, *exc):
        _lib.call("xv_set_activation", None, None)
        return False


def prelu_forward(x2d, alpha):
    """x > 0 ? x : alpha[c] * x over the last axis."""
    y = torch.empty_like(x2d)
    _lib.call("xv_prelu_forward", _s(), _p(x2d), x2d.shape[0], x2d.shape[1], _p(alpha), _p(y))
    return y


def relu_backward(da, a):
    dz = torch.empty_like(da)
    _lib.call("xv_relu_backward", _s(), _p(da), _p(a), C.c_size_t(da.numel()), _p(dz))
    return dz


def stat_pool_forward(x):
    b, t, c = x.shape
    out = _f32((b, 2 * c), x)
    _lib.call("xv_stat_pool_forward", _s(), _p(x), b, t, c, _p(out))
    return out


def stat_pool_forward_bn(z, b, t, scale, shift, relu=True, weights=None):
    """[b, 2c] statistics of relu?(z*scale+shift) without materialising it (z: [b*t, c]); weights [b, t]: self-attention."""
    c = z.shape[1]
    out = _f32((b, 2 * c), z)
    _lib.call("xv_stat_pool_forward_bn", _s(), _p(z), b, t, c, _p(scale), _p(shift), int(relu), _p(weights), _p(out))
    return out


def stat_pool_forward_bn_aux(z, b, t, scale, shift, relu=True, weights=None):
    """stat_pool_forward_bn that also returns wpos, amax [b, c] (see xv_stat_pool_forward_bn_aux)."""
    c = z.shape[1]
    out, wpos, amax = _f32((b, 2 * c), z), _f32((b, c), z), _f32((b, c), z)
    _lib.call("xv_stat_pool_forward_bn_aux", _s(), _p(z), b, t, c, _p(scale), _p(shift), int(relu), _p(weights), _p(out), _p(wpos), _p(amax))
    return out, wpos, amax


def att_score(zk, act, query, scale):
    rows, n = zk.shape
    score = _f32((rows,), zk)
    _lib.call("xv_att_score", _s(), _p(zk), rows, n, n, int(act), _p(query), float(scale), _p(score))
    return score


def key_activation(z, act):
    """act(z) with the key-layer codes: 0 identity, 1 relu, 3 tanh."""
    y = torch.empty_like(z)
    _lib.call("xv_key_activation", _s(), _p(z), C.c_size_t(z.numel()), int(act), _p(y))
    return y


def softmax_segments(score, b, t):
    w = _f32((b, t), score)
    _lib.call("xv_softmax_segments", _s(), _p(score), b, t, _p(w))
    return w


def softmax_segments_backward(w, dw):
    b, t = w.shape
    ds = _f32((b, t), w)
    _lib.call("xv_softmax_segments_backward", _s(), _p(w), _p(dw), b, t, _p(ds))
    return ds


def att_pool_backward_weights(z, b, t, scale, shift, relu, pool_out, dpool):
    c = z.shape[1]
    dw = _f32((b, t), z)
    _lib.call("xv_att_pool_backward_weights", _s(), _p(z), b, t, c, _p(scale), _p(shift), int(relu), _p(pool_out), _p(dpool), _p(dw))
    return dw


def att_key_backward(zk, act, query, scale, dscore):
    rows, n = zk.shape
    dzk, dq, db = _f32((rows, n), zk), _f32((n,), zk), _f32((n,), zk)
    wp, wb = _ws(zk)
    _lib.call("xv_att_key_backward", _s(), _p(zk), rows, n, int(act), _p(query), float(scale), _p(dscore), _p(dzk), _p(dq), _p(db), wp, wb)
    return dzk, dq, db


# ---- GhostVLAD / NetVLAD pooling (csrc/xv_vlad.hip; model/pooling.py:195-277) ----
def _vlad_shapes(name, x, a, centers, k):
    """(b, t, c, kg) of x [b, t, c], a [b*t, kg] and centers [kg, c], all contiguous float32; 1 <= k <= kg <= 64, c a multiple of 4."""
    if x.dim() != 3 or x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError("%s: x must be a contiguous float32 [batch, length, dim] tensor" % name)
    b, t, c = x.shape
    kg = int(centers.shape[0])
    f32_values(centers, kg * c, "%s: centers [%d, %d]" % (name, kg, c))
    f32_values(a, b * t * kg, "%s: the assignment weights [%d, %d]" % (name, b * t, kg))
    if c % 4 != 0 or not 1 <= int(k) <= kg <= 64:
        raise ValueError("%s: dim %d must be a multiple of 4 and 1 <= centers %d <= clusters %d <= 64" % (name, c, int(k), kg))
    return b, t, c, kg


def vlad_repitch(src, ldd):
    """src [rows, cols] (contiguous rows) as a new [rows, ldd] buffer: the first min(cols, ldd) columns, zeros behind them."""
    rows, lds = pitched(src, "vlad_repitch: src")
    if int(ldd) < 1:
        raise ValueError("vlad_repitch: the new row pitch must be positive")
    dst = _f32((rows, int(ldd)), src)
    _lib.call("xv_vlad_repitch", _s(), _p(src), rows, min(src.shape[1], int(ldd)), lds, _p(dst), int(ldd))
    return dst


def vlad_softmax(logits, kg):
    """softmax over the first kg <= 64 columns of every row of logits [rows, >= kg] (GEMM padding columns are not read) -> [rows, kg]."""
    rows, ld = pitched(logits, "vlad_softmax: logits")
    if not 1 <= int(kg) <= min(64, logits.shape[1]):
        raise ValueError("vlad_softmax: 1 <= clusters %d <= min(64, %d columns)" % (int(kg), logits.shape[1]))
    a = _f32((rows, int(kg)), logits)
    _lib.call("xv_vlad_softmax", _s(), _p(logits), rows, int(kg), ld, _p(a))
    return a


def vlad_pool_forward(x, a, centers, k, frames=None, shrink=0):
    """x [b, t, c], a [b*t, kg], centers [kg, c] -> (r [b, k, c] = sum_t a (x - c_k), n [b, k] = sum_t a) over the first k clusters;
    frames (int32 device [b]) / shrink: chunk i pools its first frames[i] - shrink rows only."""
    b, t, c, kg = _vlad_shapes("vlad_pool_forward", x, a, centers, k)
    if frames is not None and (frames.dtype != torch.int32 or frames.numel() != b or not frames.is_cuda or not frames.is_contiguous()):
        raise ValueError("vlad_pool_forward: frames must be a contiguous int32 device tensor of %d entries" % b)
    r, n = _f32((b, int(k), c), x), _f32((b, int(k)), x)
    _lib.call("xv_vlad_pool_forward", _s(), _p(x), _p(a), _p(centers), b, t, c, int(k), kg, _p(frames), int(shrink), _p(r), _p(n))
    return r, n


def vlad_normalize_forward(r, final_l2_norm):
    """r [b, k, c] -> [b, k*c]: every residual l2-normalised (epsilon 1e-12 on the squared norm), then - final_l2_norm - the whole row."""
    if r.dim() != 3 or r.dtype != torch.float32 or not r.is_contiguous() or r.shape[2] % 4 != 0 or not 1 <= r.shape[1] <= 64:
        raise ValueError("vlad_normalize_forward: r must be a contiguous float32 [batch, 1..64 centers, dim % 4 == 0] tensor")
    b, k, c = r.shape
    out = _f32((b, k * c), r)
    _lib.call("xv_vlad_normalize_forward", _s(), _p(r), b, k, c, int(bool(final_l2_norm)), _p(out))
    return out


def vlad_normalize_backward(r, dout, final_l2_norm):
    if r.dim() != 3 or r.dtype != torch.float32 or not r.is_contiguous() or r.shape[2] % 4 != 0 or not 1 <= r.shape[1] <= 64:
        raise ValueError("vlad_normalize_backward: r must be a contiguous float32 [batch, 1..64 centers, dim % 4 == 0] tensor")
    b, k, c = r.shape
    f32_values(dout, b * k * c, "vlad_normalize_backward: dout [%d, %d]" % (b, k * c))
    dr = torch.empty_like(r)
    _lib.call("xv_vlad_normalize_backward", _s(), _p(r), _p(dout), b, k, c, int(bool(final_l2_norm)), _p(dr))
    return dr


def vlad_pool_backward(x, a, centers, dr):
    """-> (da [b*t, kg] = (x - c_k) . dr_k for the k centres of dr [b, k, c], 0 for the ghosts; dx [b, t, c] = sum_k a dr_k)."""
    k = int(dr.shape[1]) if dr.dim() == 3 else 0
    b, t, c, kg = _vlad_shapes("vlad_pool_backward", x, a, centers, k)
    f32_values(dr, b * k * c, "vlad_pool_backward: dr [%d, %d, %d]" % (b, k, c))
    da, dx = _f32((b * t, kg), x), torch.empty_like(x)
    _lib.call("xv_vlad_pool_backward", _s(), _p(x), _p(a), _p(centers), _p(dr), b, t, c, k, kg, _p(da), _p(dx))
    return da, dx


def vlad_softmax_backward(a, da, ld=None):
    """dl = a (da - sum_j a da) as [rows, ld] (ld: kg rounded up to 4, the pitch of a GEMM operand; the padding columns are zero)."""
    if a.dim() != 2 or not 1 <= a.shape[1] <= 64:
        raise ValueError("vlad_softmax_backward: a must be [rows, 1..64 clusters]")
    rows, kg = a.shape
    f32_values(a, rows * kg, "vlad_softmax_backward: a")
    f32_values(da, rows * kg, "vlad_softmax_backward: da")
    ld = pitch4(kg) if ld is None else int(ld)
    if not kg <= ld <= 64:
        raise ValueError("vlad_softmax_backward: the row pitch %d must lie in %d .. 64" % (ld, kg))
    dl = _f32((rows, ld), a)
    _lib.call("xv_vlad_softmax_backward", _s(), _p(a), _p(da), rows, kg, ld, _p(dl))
    return dl


def vlad_centers_backward(n, dr, centers, l2_scale=0.0):
    """dc [kg, c] = -sum_b n[b, k] dr[b, k] for the k centres of dr [b, k, c], 0 for the ghosts, + l2_scale * centers."""
    if dr.dim() != 3 or dr.dtype != torch.float32 or not dr.is_contiguous() or centers.dim() != 2:
        raise ValueError("vlad_centers_backward: dr must be a contiguous float32 [batch, centers, dim] tensor and centers [clusters, dim]")
    b, k, c = dr.shape
    kg = int(centers.shape[0])
    f32_values(centers, kg * c, "vlad_centers_backward: centers [%d, %d]" % (kg, c))
    f32_values(n, b * k, "vlad_centers_backward: n [%d, %d]" % (b, k))
    if c % 4 != 0 or not 1 <= k <= kg <= 64:
        raise ValueError("vlad_centers_backward: dim %d must be a multiple of 4 and 1 <= centers %d <= clusters %d <= 64" % (c, k, kg))
    dc = torch.empty_like(centers)
    _lib.call("xv_vlad_centers_backward", _s(), _p(n), _p(dr), _p(centers), b, k, kg, c, float(l2_scale), _p(dc))
    return dc


def bn_relu_backward_pooled(pool_out, dpool, b, t, z, gamma, mean, invstd, scale, shift, relu=True, weights=None):
    """BN(+ReLU) backward of the layer feeding statistics pooling, upstream gradient = pooling backward on the fly."""
    n = z.shape[1]
    dz = _f32((b * t, n), z)
    dgamma, dbeta, dbias = _f32((n,), z), _f32((n,), z), _f32((n,), z)
    wp, wb = _ws(z)
    _lib.call("xv_bn_relu_backward_pooled", _s(), _p(pool_out), _p(dpool), _p(weights), b, t, _p(z), n, _p(gamma), _p(mean), _p(invstd), _p(scale),
              _p(shift), int(relu), _p(dz), _p(dgamma), _p(dbeta), _p(dbias), wp, wb)
    return dz, dgamma, dbeta, dbias


def bn_relu_backward_pooled_aux(pool_out, dpool, wpos, b, t, z, gamma, mean, invstd, scale, shift, relu=True, weights=None):
    """bn_relu_backward_pooled with the reductions in closed form from (pool_out, dpool, wpos): no reduction pass over z."""
    n = z.shape[1]
    dz = _f32((b * t, n), z)
    dgamma, dbeta, dbias = _f32((n,), z), _f32((n,), z), _f32((n,), z)
    wp, wb = _ws(z)
    _lib.call("xv_bn_relu_backward_pooled_aux", _s(), _p(pool_out), _p(dpool), _p(weights), _p(wpos), b, t, _p(z), n, _p(gamma), _p(mean),
              _p(invstd), _p(scale), _p(shift), int(relu), _p(dz), _p(dgamma), _p(dbeta), _p(dbias), wp, wb)
    return dz, dgamma, dbeta, dbias


def stat_pool_backward(x, out, dout):
    b, t, c = x.shape
    dx = torch.empty_like(x)
    _lib.call("xv_stat_pool_backward", _s(), _p(x), _p(out), _p(dout), b, t, c, _p(dx))
    return dx


def l2_scaling_forward(x, factor):
    y = torch.empty_like(x)
    _lib.call("xv_l2_scaling_forward", _s(), _p(x), x.shape[0], x.shape[1], float(factor), _p(y))
    return y


def l2_scaling_backward(x, dy, factor):
    dx = torch.empty_like(x)
    _lib.call("xv_l2_scaling_backward", _s(), _p(x), _p(dy), x.shape[0], x.shape[1], float(factor), _p(dx))
    return dx


def loss_prep_weight(w, normalize):
    c, n = w.shape
    ldn = pitch4(n)
    inv = _f32((n,), w)
    wn = _f32((c, ldn), w)
    wnt = _f32((n, c), w)
    _lib.call("xv_loss_prep_weight", _s(), _p(w), c, n, int(normalize), _p(inv), _p(wn), ldn, _p(wnt))
    return inv, wn, wnt


def margin_softmax_rows(kind, logits, n, x, labels, m, lam):
    """logits: [rows, ldl] (ldl >= n).  Returns loss (1-elem tensor), dlogits, dnorm, row_loss."""
    rows, ldl = logits.shape
    dlogits = torch.empty_like(logits)
    dnorm, row_loss, loss = _f32((rows,), logits), _f32((rows,), logits), _f32((1,), logits)
    _lib.call("xv_margin_softmax_rows", _s(), int(kind), _p(logits), rows, n, ldl, _p(x), x.shape[1], _p(labels), float(m),
              float(lam), _p(dlogits), _p(dnorm), _p(row_loss), _p(loss))
    return loss, dlogits, dnorm, row_loss


def pair_loss_config(loss_func, margin=0.0, squared=False, triplet_type="all", loss_type="additive_margin_softmax", valid_speakers=0,
                     valid_segments=0):
    """The xv_pair_loss_config of "semihard_triplet_loss" / "angular_triplet_loss" with the reference's option names (loss.py:376-377, 509-511)."""
    head = kinds.loss(loss_func, kinds.PAIR)
    head.check(margin, triplet_type, loss_type)      # what the kind refuses of these options (kinds.py)
    return _lib.XvPairLossConfig(kind=head.pair_code, squared=int(bool(squared)), triplet_type=_lib.TRIPLET_TYPES.get(triplet_type, 0),
                                 margin_kind=_lib.LOSS_KINDS.get(loss_type, 2), margin=float(margin), valid_speakers=int(valid_speakers),
                                 valid_segments=int(valid_segments))


def _pair_ws(x, d, ws):
    b, ldx = pitched(x, "pair loss: x")
    need = int(_lib.load().xv_pair_loss_workspace_bytes(b, d))
    if need == 0:
        _lib.check(2, "xv_pair_loss_workspace_bytes")
    if ws is None:
        ws = torch.empty(need // 4, dtype=torch.float32, device=x.device)
    return b, ldx, ws


def pair_loss(cfg, x, labels, d=None, ws=None):
    """x: [b, >= d] float32 view with contiguous rows (d: x.shape[1]), labels int32 [b].  -> (loss [1], stats [4], ws); ws holds what
    pair_loss_backward reads."""
    d = x.shape[1] if d is None else int(d)
    b, ldx, ws = _pair_ws(x, d, ws)
    if labels.dtype != torch.int32 or labels.numel() != b or not labels.is_contiguous():
        raise ValueError("pair loss: labels must be %d contiguous int32 values" % b)
    loss, stats = _f32((1,), x), _f32((4,), x)
    _lib.call("xv_pair_loss_forward", _s(), C.byref(cfg), _p(x), b, d, ldx, _p(labels), _p(loss), _p(stats), _p(ws), C.c_size_t(ws.numel() * 4))
    return loss, stats, ws


def pair_loss_backward(cfg, x, labels, ws, d=None, out=None):
    """d loss / d x [b, d] (or into `out`, a [b, >= d] view with contiguous rows) from the workspace pair_loss left."""
    d = x.shape[1] if d is None else int(d)
    if ws is None:
        raise ValueError("pair loss: the backward needs the workspace pair_loss returned for the same cfg, x and labels")
    b, ldx, ws = _pair_ws(x, d, ws)
    if labels.dtype != torch.int32 or labels.numel() != b or not labels.is_contiguous():
        raise ValueError("pair loss: labels must be %d contiguous int32 values" % b)
    dx = _f32((b, d), x) if out is None else out
    _, lddx = pitched(dx, "pair loss: dx")
    _lib.call("xv_pair_loss_backward", _s(), C.byref(cfg), _p(x), b, d, ldx, _p(labels), _p(ws), C.c_size_t(ws.numel() * 4), _p(dx), lddx)
    return dx


def e2e_valid_loss(x, speakers, segments, d=None, ws=None):
    """loss [1] of speakers x segments speaker-major rows (loss.py:637-705)"""
    d = x.shape[1] if d is None else int(d)
    if x.shape[0] != int(speakers) * int(segments):
        raise ValueError("e2e_valid_loss: %d rows are not %d speakers x %d segments" % (x.shape[0], speakers, segments))
    b, ldx, ws = _pair_ws(x, d, ws)
    loss = _f32((1,), x)
    _lib.call("xv_e2e_valid_loss", _s(), _p(x), int(speakers), int(segments), d, ldx, _p(loss), _p(ws), C.c_size_t(ws.numel() * 4))
    return loss


def ge2e_loss_config(ge2e_loss_type, speakers, segments, valid_speakers=0, valid_segments=0):
    """The xv_ge2e_config of "ge2e_loss" with the reference's asserts (kinds.check_ge2e: loss.py:937, 980): ge2e_loss_type "softmax" /
    "contrastive" on speakers x segments speaker-major rows."""
    kinds.loss("ge2e_loss", kinds.GE2E).check(ge2e_loss_type, segments)
    return _lib.XvGe2eConfig(loss_type=_lib.GE2E_TYPES[ge2e_loss_type], speakers=int(speakers), segments=int(segments),
                             valid_speakers=int(valid_speakers), valid_segments=int(valid_segments))


def _ge2e_args(cfg, x, w, b, d, ws):
    d = x.shape[1] if d is None else int(d)
    rows, ldx = ge2e_rows(x, cfg.speakers, cfg.segments, d)
    f32_values(w, 1, "ge2e loss: w")
    f32_values(b, 1, "ge2e loss: b")
    need = int(_lib.load().xv_ge2e_loss_workspace_bytes(cfg.speakers, cfg.segments, d))
    if need == 0:
        _lib.check(2, "xv_ge2e_loss_workspace_bytes")
    if ws is None:
        ws = torch.empty(need // 4, dtype=torch.float32, device=x.device)
    return rows, d, ldx, ws


def ge2e_loss(cfg, x, w, b, d=None, ws=None):
    """x: [speakers * segments, >= d] float32 view with contiguous rows, speaker-major (d: x.shape[1]); w, b: one device float each.
    -> (loss [1], stats [4] = {d w, d b, 0, 0}, ws); ws holds what ge2e_loss_backward reads."""
    rows, d, ldx, ws = _ge2e_args(cfg, x, w, b, d, ws)
    loss, stats = _f32((1,), x), _f32((4,), x)
    _lib.call("xv_ge2e_loss_forward", _s(), C.byref(cfg), _p(x), d, ldx, _p(w), _p(b), _p(loss), _p(stats), _p(ws), C.c_size_t(ws.numel() * 4))
    return loss, stats, ws


def ge2e_loss_backward(cfg, x, w, b, ws, d=None, out=None):
    """(d loss / d x [rows, d] - or into `out`, a [rows, >= d] view with contiguous rows -, d w [1], d b [1]) from the workspace ge2e_loss left."""
    if ws is None:
        raise ValueError("ge2e loss: the backward needs the workspace ge2e_loss returned for the same cfg, x, w and b")
    rows, d, ldx, ws = _ge2e_args(cfg, x, w, b, d, ws)
    dx = _f32((rows, d), x) if out is None else out
    _, lddx = pitched(dx, "ge2e loss: dx")
    dw, db = _f32((1,), x), _f32((1,), x)
    _lib.call("xv_ge2e_loss_backward", _s(), C.byref(cfg), _p(x), d, ldx, _p(w), _p(b), _p(ws), C.c_size_t(ws.numel() * 4), _p(dx), lddx, _p(dw), _p(db))
    return dx, dw, db


def add_norm_grad(x, dnorm, dx):
    _lib.call("xv_add_norm_grad", _s(), _p(x), _p(dnorm), x.shape[0], x.shape[1], _p(dx))
    return dx


_TICKETS = {}


def _tickets(like, n):
    """Zeroed uint32 tickets for the segment-level launches (one per 32 output columns; every launch leaves them zero)."""
    key = str(like.device)
    need = (n + 31) // 32 + 8
    if key not in _TICKETS or _TICKETS[key].numel() < need:
        _TICKETS[key] = torch.zeros(max(need, 1024), dtype=torch.int32, device=like.device)
    return _TICKETS[key]


def _row_term(row_term):
    if row_term is None:
        return _p(None), _p(None), _p(None), 0
    coef, norm, xrow = row_term
    return _p(coef), _p(norm), _p(xrow), xrow.shape[1]


def segment_gemm(a, bt, bias=None, row_term=None):
    """c[m][n] = sum_k a[m][k] bt[n][k] + bias[n] (+ (coef[m]/norm[m]) xrow[m][n]); m <= 128 rows, one launch."""
    m, k = a.shape
    n = bt.shape[0]
    c = _f32((m, n), a)
    wp, wb = _ws(a)
    rc, rn, rx, ldx = _row_term(row_term)
    _lib.call("xv_segment_gemm", _s(), _p(a), a.stride(0), _p(bt), bt.stride(0), m, n, k, _p(bias), rc, rn, rx, ldx, _p(c), n,
              wp, wb, _p(_tickets(a, n)))
    return c


def segment_affine_bn_forward(x, wt, bias, gamma, beta, eps, momentum, unbiased, moving_mean, moving_var, relu, want_a=True):
    """dense + training-mode BatchNorm (+ ReLU) on m <= 128 rows in one launch.  Returns z, a, mean, invstd, scale, shift."""
    m, k = x.shape
    n = wt.shape[0]
    z = _f32((m, n), x)
    a = _f32((m, n), x) if want_a else None
    mean, invstd, scale, shift = (_f32((n,), x) for _ in range(4))
    wp, wb = _ws(x)
    _lib.call("xv_segment_affine_bn_forward", _s(), _p(x), x.stride(0), _p(wt), wt.stride(0), m, n, k, _p(bias), _p(gamma), _p(beta),
              float(eps), float(momentum), int(unbiased), _p(moving_mean), _p(moving_var), _p(z), _p(mean), _p(invstd), _p(scale),
              _p(shift), int(relu), _p(a), wp, wb, _p(_tickets(x, n)))
    return z, a, mean, invstd, scale, shift


def segment_dgrad_bn_backward(dy, wt, z, gamma, mean, invstd, scale, shift, relu, row_term=None):
    """d a = dy . wt^T (+ row term), then the BatchNorm (+ ReLU) backward of the layer with pre-BN tensor z.  Returns dz, dgamma, dbeta, dbias."""
    m, k = dy.shape
    n = wt.shape[0]
    dz = _f32((m, n), dy)
    dgamma, dbeta, dbias = (_f32((n,), dy) for _ in range(3))
    wp, wb = _ws(dy)
    rc, rn, rx, ldx = _row_term(row_term)
    _lib.call("xv_segment_dgrad_bn_backward", _s(), _p(dy), dy.stride(0), _p(wt), wt.stride(0), m, n, k, rc, rn, rx, ldx, _p(z),
              _p(gamma), _p(mean), _p(invstd), _p(scale), _p(shift), int(relu), _p(dz), _p(dgamma), _p(dbeta), _p(dbias), wp, wb,
              _p(_tickets(dy, n)))
    return dz, dgamma, dbeta, dbias


def loss_weight_backward(dwn, wn, inv, w, normalize, l2_scale):
    c, n = w.shape
    dw = torch.empty_like(w)
    wp, wb = _ws(w)
    _lib.call("xv_loss_weight_backward", _s(), _p(dwn), dwn.stride(0), _p(wn), wn.stride(0), _p(inv), _p(w), c, n, int(normalize),
              float(l2_scale), _p(dw), wp, wb)
    return dw


def ring_loss(x, r, lam):
    """lam * mean((||x|| - r)^2) as a device scalar (loss.py:1003-1017)."""
    rows, n = x.shape
    out, dn, dr = _f32((1,), x).zero_(), _f32((rows,), x).zero_(), _f32((1,), x)
    _lib.call("xv_ring_loss", _s(), _p(x), rows, n, n, _p(r), float(lam), _p(out), _p(dn), _p(dr))
    return out[0]


def mhe_loss(wn, n, labels, lam):
    """lam / (mean_{b,n}(2 - 2 wn[:,y_b].wn[:,n]) + 1e-6) on column-normalised weights wn [c, ldn] (loss.py:1018-1033)."""
    c, ldn = wn.shape
    out, coef = _f32((1,), wn).zero_(), _f32((1 + 2 * c,), wn)
    counts = torch.empty(n, dtype=torch.int32, device=wn.device)
    _lib.call("xv_mhe_loss", _s(), _p(wn), c, n, ldn, _p(labels), labels.shape[0], float(lam), _p(out), _p(coef), _p(counts))
    return out[0]


def l2_reg_loss(w, scale, accum):
    _lib.call("xv_l2_reg_loss", _s(), _p(w), C.c_size_t(w.numel()), float(scale), _p(accum))


def sumsq(g, accum):
    _lib.call("xv_sumsq", _s(), _p(g), C.c_size_t(g.numel()), _p(accum))


def sgd_update(p, g, lr, grad_scale=1.0):
    _lib.call("xv_sgd_update", _s(), _p(p), _p(g), C.c_size_t(p.numel()), float(lr), float(grad_scale))


def momentum_update(p, g, acc, lr, momentum, nesterov, grad_scale=1.0):
    _lib.call("xv_momentum_update", _s(), _p(p), _p(g), _p(acc), C.c_size_t(p.numel()), float(lr), float(momentum), int(nesterov),
              float(grad_scale))


def adam_update(p, g, m, v, lr, t, beta1=0.9, beta2=0.999, eps=1e-8, grad_scale=1.0):
    _lib.call("xv_adam_update", _s(), _p(p), _p(g), _p(m), _p(v), C.c_size_t(p.numel()), float(lr), float(beta1), float(beta2),
              float(eps), int(t), float(grad_scale))


# ---- split precision (f16x3): fp32 tensors as two fp16 planes + a device-side max |x| -------------------------
class Planes(object):
    """[2][rows][ld] fp16 planes of an fp32 matrix plus the uint32 float-bits of its max |x| (device)."""

    def __init__(self, data, rows, ld, amax):
        self.data, self.rows, self.ld, self.amax = data, rows, ld, amax

    @property
    def stride(self):
        return self.rows * self.ld


def amax_of(x):
    a = torch.zeros(1, dtype=torch.int32, device=x.device)
    _lib.call("xv_amax", _s(), _p(x), C.c_size_t(x.numel()), _p(a))
    return a


def split_planes(x2d, amax=None):
    rows, c = x2d.shape
    ld = (c + 7) // 8 * 8
    if amax is None:
        amax = amax_of(x2d)
    data = torch.empty((2, rows, ld), dtype=torch.int16, device=x2d.device)
    _lib.call("xv_split_planes", _s(), _p(x2d), rows, c, x2d.stride(0), _p(data), ld, C.c_size_t(rows * ld), _p(amax))
    return Planes(data, rows, ld, amax)


def bn_apply_split(z, scale, shift, relu, amax):
    rows, n = z.shape
    ld = (n + 7) // 8 * 8
    data = torch.empty((2, rows, ld), dtype=torch.int16, device=z.device)
    _lib.call("xv_bn_apply_split", _s(), _p(z), rows, n, n, _p(scale), _p(shift), int(relu), _p(amax), _p(data), ld, C.c_size_t(rows * ld))
    return Planes(data, rows, ld, amax)


def bn_relu_backward_split(da, z, segs, t, gamma, mean, invstd, scale, shift, zmin, zmax, relu, pad):
    n = z.shape[1]
    ld = (n + 7) // 8 * 8
    rows = segs * (t + 2 * pad)
    data = torch.empty((2, rows, ld), dtype=torch.int16, device=z.device)
    amax = torch.zeros(1, dtype=torch.int32, device=z.device)
    dgamma, dbeta, dbias = _f32((n,), z), _f32((n,), z), _f32((n,), z)
    wp, wb = _ws(z)
    _lib.call("xv_bn_relu_backward_split", _s(), _p(da), _p(z), segs, t, n, _p(gamma), _p(mean), _p(invstd), _p(scale), _p(shift),
              _p(zmin), _p(zmax), int(relu), int(pad), _p(data), ld, C.c_size_t(rows * ld), _p(amax), _p(dgamma), _p(dbeta), _p(dbias),
              wp, wb)
    return Planes(data, rows, ld, amax), dgamma, dbeta, dbias


def bn_relu_backward_pooled_split(pool_out, dpool, b, t, z, gamma, mean, invstd, scale, shift, zmin, zmax, relu=True, weights=None):
    n = z.shape[1]
    ld = (n + 7) // 8 * 8
    rows = b * t
    data = torch.empty((2, rows, ld), dtype=torch.int16, device=z.device)
    amax = torch.zeros(1, dtype=torch.int32, device=z.device)
    dgamma, dbeta, dbias = _f32((n,), z), _f32((n,), z), _f32((n,), z)
    wp, wb = _ws(z)
    _lib.call("xv_bn_relu_backward_pooled_split", _s(), _p(pool_out), _p(dpool), _p(weights), b, t, _p(z), n, _p(gamma), _p(mean), _p(invstd), _p(scale),
              _p(shift), _p(zmin), _p(zmax), int(relu), _p(data), ld, C.c_size_t(rows * ld), _p(amax), _p(dgamma), _p(dbeta), _p(dbias),
              wp, wb)
    return Planes(data, rows, ld, amax), dgamma, dbeta, dbias


def affine_forward_f16x3(xp, segs, t_in, k, wtp, bias, o, with_stats=False, ldz=None):
    """xp: Planes of x [segs*t_in][c_ld]; wtp: Planes of Wt [o][k*c_ld]; ldz: the row pitch of z in floats (default o: contiguous)."""
    rows = segs * (t_in - k + 1)
    ldz = o if ldz is None else ldz
    z = torch.empty((rows, ldz), dtype=torch.float32, device=xp.data.device)[:, :o]
    part = torch.empty((4, (rows + TILE_M - 1) // TILE_M, o), dtype=torch.float32, device=z.device) if with_stats else None
    _lib.call("xv_affine_forward_f16x3", _s(), _p(xp.data), C.c_size_t(xp.stride), _p(xp.amax), segs, t_in, xp.ld, k, _p(wtp.data),
              C.c_size_t(wtp.stride), _p(wtp.amax), _p(bias), _p(z), o, ldz, _p(part))
    return (z, part) if with_stats else z


def affine_dgrad_f16x3(dzp, segs, t_out, k, wfp, c):
    dx = torch.empty((segs * (t_out + k - 1), c), dtype=torch.float32, device=dzp.data.device)
    _lib.call("xv_affine_dgrad_f16x3", _s(), _p(dzp.data), C.c_size_t(dzp.stride), _p(dzp.amax), segs, t_out, dzp.ld, k, _p(wfp.data),
              C.c_size_t(wfp.stride), _p(wfp.amax), _p(dx), c)
    return dx


def affine_dgrad_bnstats_f16x3(dzp, segs, t_out, k, wfp, c, z_below, scale, shift, mean, invstd):
    """affine_dgrad_f16x3 + the per-tile BN-backward partials [ceil(rows/128), 3, c] of the layer that owns dx."""
    rows = segs * (t_out + k - 1)
    dx = torch.empty((rows, c), dtype=torch.float32, device=dzp.data.device)
    part = torch.empty(((rows + TILE_M - 1) // TILE_M, 3, c), dtype=torch.float32, device=dx.device)
    _lib.call("xv_affine_dgrad_bnstats_f16x3", _s(), _p(dzp.data), C.c_size_t(dzp.stride), _p(dzp.amax), segs, t_out, dzp.ld, k, _p(wfp.data),
              C.c_size_t(wfp.stride), _p(wfp.amax), _p(dx), c, _p(z_below), _p(scale), _p(shift), _p(mean), _p(invstd), _p(part))
    return dx, part


def affine_wgrad_f16x3(xp, segs, t_in, k, c, dzp, dz_seg_pitch, dz_row0, o, kernel, l2_scale):
    dk = torch.empty((k, c, o), dtype=torch.float32, device=xp.data.device)
    wp, wb = _ws(dk)
    _lib.call("xv_affine_wgrad_f16x3", _s(), _p(xp.data), C.c_size_t(xp.stride), _p(xp.amax), segs, t_in, xp.ld, k, c, _p(dzp.data),
              C.c_size_t(dzp.stride), _p(dzp.amax), dz_seg_pitch, dz_row0, dzp.ld, o, _p(kernel), float(l2_scale), _p(dk), wp, wb)
    return dk
