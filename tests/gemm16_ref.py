"""NumPy model of the split-precision (f16x3) representation and GEMMs of csrc/xv_gemm16.h (xv_planes16.hip, xv_gemm16_nt.hip, xv_gemm16_tn.hip) with the bound of each output, what
tests/test_gpu_gemm16_forms.py compares the kernels with.  As in tests/segment_ref.py: float64 is the reference, class NumpyOps is a plain
float32 NumPy evaluation of the same formulas behind the interface of the GPU backend, which tests/test_gemm16_ref.py holds against the same
bounds before the kernels run; u = 2^-24; bounds are per element or per channel, never relative to a tensor's largest entry.

Planes.  A tensor with max |x| = amax is carried as h = fp16(x s), l = fp16(x s - h) with s the power of two that brings amax into
[2^12, 2^13) (pow2_scale: the float bits of amax exactly as xv_pow2_scale reads them).  x s is exact (a power of two; no overflow or
underflow for |12 - e| <= 100), x s - h is exact in float32 (h is x s rounded to 11 bits), both roundings are float32 -> float16 to
nearest even with subnormals kept - NumPy's astype.  The device planes are compared with this model bit for bit.  Compiled for gfx950 the
emitters form h with v_cvt_pk_f16_f32 and l with v_fma_mix{lo,hi}_f16 (x s - h in one operation, rounded once: the same value, since the
difference is exact), and xv_bn_apply_split forms z scale + shift with v_pk_fma_f32: ONE fused operation (R.fma32), then the activation (a
slope's product rounds once), then the split - so its planes have no ambiguous elements either.

Representation error of an element: eps(x) = max(2^-22 |x|, 2^-25 / s): h keeps 11 bits, l another 11 of the remainder unless it is a
subnormal fp16 (quantum 2^-24: half of it); 0 for x = 0.

GEMM bound, per output element with S = sum_k |a_k| |b_k|:
  representation      sum_k |a| eps(b) + eps(a) |b| + eps(a) eps(b)
  the dropped l.l     |la lb| / (sa sb) <= 2^-11 |a| 2^-11 |b| per term: 2^-22 S
  accumulation        products of two fp16 are exact in fp32.  A form chains L matrix instructions on one accumulator: three (h.l, l.h, h.h) per
                      block of KK = 16 (generic kernel: two blocks per 32-half K-step) or 32 (context-window and TN kernels: one) reduction
                      indices.  Each addition onto the accumulator rounds once (u times the partial sum, which is at most S (1 + 2^-10));
                      inside an instruction the KK exact products are summed in an order the ISA does not state - any order of fp32
                      additions is within (KK - 1) u of the sum of their magnitudes, and the instructions' magnitudes add up to S (1 + 2^-10).
                      Together (L + KK) u S (1 + 2^-10).
  scaling             by 1 / (sa sb), a power of two: exact.  Bias: acc * scale + bias rounds once: u |result|.
  TN                  the slabs of the splits are added in split order (xv_launch_wgrad_reduce, either form: at most `splits` additions on
                      a chain), + l2 * w rounds twice at most: (splits + 2) u (S + |l2 w|).
The bounds are loose by construction where the chain is long (worst-case signs against random ones); the ledger shows the ratio."""
import numpy as np

import bn_pool_ref as R
import test_gemm16_plans as P
from bn_pool_ref import U, f32, f64
from oracle import xvector_oracle as O

Q16 = 2.0 ** -24                                  # the fp16 subnormal quantum
EPI_L = {P.GENERIC: 32 + 1 + 1, P.CONV: 16 + 2 + 1}      # column reductions of the epilogues: a lane's rows in order, the lane combine, the two row-waves
MFMA_K = {P.GENERIC: 16, P.CONV: 32, "tn": 32}           # reduction indices one matrix instruction spans


# ------------------------------------------------------------------ planes
def bits_of(v):
    return int(np.array([v], np.float32).view(np.uint32)[0])


def float_of(bits):
    return np.array([bits], np.uint32).view(np.float32)[0]


def pow2_scale(amax_bits):
    """xv_pow2_scale: 1 for amax = 0, inf or nan; else 2^(12 - e) with e the biased exponent field - 127, 12 - e clamped to +-100."""
    amax = float_of(amax_bits)
    if not (amax > 0) or not (amax < np.inf):
        return np.float32(1)
    s = max(-100, min(100, 12 - (((int(amax_bits) >> 23) & 0xff) - 127)))
    return float_of((s + 127) << 23)


def amax_bits(x, prev=0):
    """xv_amax: the float bits of max |x|, accumulated onto a previous value as unsigned integers (non-negative floats order like their bits)."""
    x = f32(x)
    return max(int(prev), bits_of(np.abs(x).max()) if x.size else 0)


def split(x, bits, ld=None):
    """[2][rows][ld] uint16: the planes of x [rows][c] at the scale of amax bits; columns c ... ld are zero."""
    x = f32(x)
    rows, c = x.shape
    ld = P.align8(c) if ld is None else ld
    xs = x * pow2_scale(bits)
    out = np.zeros((2, rows, ld), np.float16)
    with np.errstate(over="ignore", invalid="ignore"):
        out[0, :, :c] = xs.astype(np.float16)
        out[1, :, :c] = (xs - out[0, :, :c].astype(np.float32)).astype(np.float16)
    return out.view(np.uint16)


def plane_values(planes):
    """uint16 planes -> float32 values of h and l"""
    p = np.ascontiguousarray(planes).view(np.float16).astype(np.float32)
    return p[0], p[1]


def eps_rep(x, bits):
    ax = np.abs(f64(x))
    return np.where(ax == 0, 0.0, np.maximum(2.0 ** -22 * ax, 0.5 * Q16 / float(pow2_scale(bits))))


def bn_apply_value(z, scale, shift, relu, slope):
    """The float32 value xv_bn_apply_split splits: fma(z, scale, shift), then relu ? (y > 0 ? y : slope y) : y with a float32 product."""
    y = R.fma32(z, np.asarray(scale, np.float32)[None, :], np.asarray(shift, np.float32)[None, :])
    if not relu:
        return y
    if slope is None:
        return np.maximum(y, np.float32(0))
    return np.where(y > 0, y, y * np.asarray(slope, np.float32)[None, :]).astype(np.float32)


# ------------------------------------------------------------------ operands
def make_operands(rs, segs, t_in, c, k, o):
    """ReLU-like activations x 1.7, weights 1 / sqrt(K), bias randn, gradients around 3e-4 with one entry 1e4 times the typical value."""
    t_out = t_in - k + 1
    x = f32(np.maximum(rs.randn(segs, t_in, c), 0) * 1.7)
    kern = f32(rs.randn(k, c, o) / np.sqrt(k * c))
    bias = f32(rs.randn(o))
    dz = rs.randn(segs, t_out, o) * 3e-4
    dz[segs // 2, t_out // 2, o // 3] = 3.0
    return x, kern, bias, f32(dz)


def _hash(shape, salt):
    idx = np.arange(int(np.prod(shape)), dtype=np.uint64).reshape(shape)
    return ((idx * np.uint64(2654435761) + np.uint64(salt * 40503 + 12345)) % np.uint64(1 << 32)) >> np.uint64(5)


def coded_wide(shape, terms, salt):
    """Position-coded integers of up to 20 bits (pieces h and l both in use) with 3 |v| terms <= 2^23: against coded_small every product and
    every partial sum of `terms` of them, in any order, is an integer below 2^24 - exact in fp32."""
    mag = min(1 << 20, 1 << int(np.floor(np.log2((1 << 23) / (3.0 * terms)))))
    return f32((_hash(shape, salt) % np.uint64(2 * mag - 1)).astype(np.int64) - (mag - 1))


def coded_small(shape, salt):
    """Position-coded integers in {-3, -2, -1, 1, 2, 3}: one piece (l = 0), so that no l.l product is dropped."""
    v = (_hash(shape, salt) % np.uint64(6)).astype(np.int64)
    return f32(np.where(v < 3, v - 3, v - 2))


# ------------------------------------------------------------------ references and bounds
def nt_chain(form):
    """(L, KK) of an NT form (P.nt_form): matrix instructions chained on an accumulator, reduction indices of one."""
    kernel, nk = form[0], form[6]
    return 3 * nk * (32 // MFMA_K[kernel]), MFMA_K[kernel]


def tn_chain(plan):
    """(L, KK, splits) of a TN plan (P.tn_plan): a split chains the stages of its r_chunk rows."""
    return 3 * (plan[2] // 32), MFMA_K["tn"], plan[1]


def _abs_conv(x, kern):
    return O.conv1d_valid_fwd(x, kern, np.zeros(kern.shape[2]))


def forward(x, kern, bias):
    b = np.zeros(kern.shape[2]) if bias is None else f64(bias)
    return O.conv1d_valid_fwd(f64(x), f64(kern), b).reshape(-1, kern.shape[2])


def gemm_terms(a, ea, b, eb, contract):
    """S and the representation term of a contraction `contract(a, b)` that is bilinear in two non-negative operands"""
    return contract(a, b), contract(a, eb) + contract(ea, b) + contract(ea, eb)


def accumulate_bound(S, rep, L, kk):
    return rep + 2.0 ** -22 * S + (L + kk) * U * S * (1 + 2.0 ** -10)


def forward_bound(x, kern, bias, ax, aw, form):
    o = kern.shape[2]
    S, rep = gemm_terms(np.abs(f64(x)), eps_rep(x, ax), np.abs(f64(kern)), eps_rep(kern, aw), lambda a, b: _abs_conv(a, b).reshape(-1, o))
    ref = forward(x, kern, bias)
    return ref, (accumulate_bound(S, rep, *nt_chain(form)) + U * np.abs(ref)) * (1 + 1e-3)


def dgrad(dz, kern, t_in):
    segs = dz.shape[0]
    x0 = np.zeros((segs, t_in, kern.shape[1]))
    return O.conv1d_valid_bwd(x0, f64(kern), f64(dz))[0].reshape(-1, kern.shape[1])


def dgrad_bound(dz, kern, t_in, adz, aw, form):
    c = kern.shape[1]
    x0 = np.zeros((dz.shape[0], t_in, c))
    S, rep = gemm_terms(np.abs(f64(dz)), eps_rep(dz, adz), np.abs(f64(kern)), eps_rep(kern, aw),
                        lambda a, b: O.conv1d_valid_bwd(x0, b, a)[0].reshape(-1, c))
    ref = dgrad(dz, kern, t_in)
    return ref, (accumulate_bound(S, rep, *nt_chain(form)) + U * np.abs(ref)) * (1 + 1e-3)


def wgrad(x, dz, kern, l2):
    k0 = np.zeros(kern.shape)
    return O.conv1d_valid_bwd(f64(x), k0, f64(dz))[1] + float(np.float32(l2)) * f64(kern)


def wgrad_bound(x, dz, kern, l2, ax, adz, plan):
    k0 = np.zeros(kern.shape)
    S, rep = gemm_terms(np.abs(f64(x)), eps_rep(x, ax), np.abs(f64(dz)), eps_rep(dz, adz), lambda a, b: O.conv1d_valid_bwd(a, k0, b)[1])
    L, kk, splits = tn_chain(plan)
    reg = np.abs(float(np.float32(l2)) * f64(kern))
    return wgrad(x, dz, kern, l2), (accumulate_bound(S, rep, L, kk) + (splits + 2) * U * (S + reg)) * (1 + 1e-3)


def tile_stats(z, kernel):
    """The [4][tiles of 128 rows][n] statistics of the forward epilogues on the float32 z the launch returned, with the bounds of the sum and
    of the centred squares (R.col_stats_bound at the epilogue's chain: EPI_L); min and max are exact."""
    ref = R.col_stats(f64(z))
    b, _ = R.col_stats_bound(z, EPI_L[kernel])
    return ref, b


def bwd_partials(dx, z, scale, shift, mean, invstd, dt=np.float64):
    """[tiles][3][n] of the data-gradient epilogue on the dx the launch returned: sum dd | sum dd xhat | max |dd| per 128-row tile,
    dd = (z scale + shift > 0) ? dx : 0, xhat = (z - mean) invstd."""
    dx, z = np.asarray(dx, dt), np.asarray(z, dt)
    sc, sh, mu, istd = (np.asarray(v, dt) for v in (scale, shift, mean, invstd))
    dd = np.where(z * sc + sh > 0, dx, dt(0))
    xh = (z - mu) * istd
    T = R.tiles_of(dx.shape[0])
    out = np.zeros((T, 3, dx.shape[1]), dt)
    for t in range(T):
        r = slice(128 * t, 128 * t + 128)
        out[t, 0], out[t, 1], out[t, 2] = R.rsum(dd[r], 0, dt), R.rsum(dd[r] * xh[r], 0, dt), np.abs(dd[r]).max(axis=0)
    return out


def bwd_partials_bound(dx, z, scale, shift, mean, invstd):
    """-> (ref, bound [tiles][2][n], ambiguous mask, keep [tiles][n]: tiles of a column without an ambiguous element).  Chain EPI_L[generic]; a
    term of sum dd is exact, of sum dd xhat carries 3 roundings (the difference, two products); an element whose mask is ambiguous
    (R.pre_activation) may enter or leave: its |dx| (|dx xhat|) is added to the bound, and max |dd| is compared where no element is."""
    ref = bwd_partials(dx, z, scale, shift, mean, invstd)
    _, _, amb, _ = R.pre_activation(z, scale, shift)
    dxa = np.abs(f64(dx))
    xh = np.abs((f64(z) - f64(mean)) * f64(invstd))
    dd = np.where(f64(z) * f64(scale) + f64(shift) > 0, dxa, 0.0)
    L = EPI_L[P.GENERIC]
    T = ref.shape[0]
    b, keep = np.zeros((T, 2, dx.shape[1])), np.zeros((T, dx.shape[1]), bool)
    for t in range(T):
        r = slice(128 * t, 128 * t + 128)
        b[t, 0] = L * U * dd[r].sum(axis=0) + (dxa[r] * amb[r]).sum(axis=0)
        b[t, 1] = (L + 3) * U * (dd[r] * xh[r]).sum(axis=0) + (dxa[r] * xh[r] * amb[r]).sum(axis=0)
        keep[t] = ~amb[r].any(axis=0)
    return ref, b, amb, keep


# ------------------------------------------------------------------ the same interface as the GPU backend, in plain float32 NumPy
def spliced(v, k):
    """[segs][t][c] -> [segs * (t - k + 1)][k * c]: row (segment, frame) is the k frames from it on, tap-major."""
    segs, t, c = v.shape
    t_out = t - k + 1
    return np.concatenate([v[:, j:j + t_out, :] for j in range(k)], axis=2).reshape(segs * t_out, k * c)


def padded(dz, pad):
    return np.pad(dz, ((0, 0), (pad, pad), (0, 0)))


def weights_fwd(kern, c_ld):
    """wt[o][j * c_ld + ch] = kern[j][ch][o]"""
    k, c, o = kern.shape
    w = np.zeros((o, k, c_ld), np.float32)
    w[:, :, :c] = np.transpose(kern, (2, 0, 1))
    return w.reshape(o, k * c_ld)


def weights_dgrad(kern, o_ld):
    """wf[ch][(k - 1 - j) * o_ld + o] = kern[j][ch][o]"""
    k, c, o = kern.shape
    w = np.zeros((c, k, o_ld), np.float32)
    w[:, :, :o] = np.transpose(kern[::-1], (1, 0, 2))
    return w.reshape(c, k * o_ld)


class NumpyOps(object):
    """The planes of the model, the three products of a block in float32 matrix products, float32 accumulation in the form's block order."""
    name = "numpy-float32"

    def amax(self, x, prev=0, offset=0):
        return amax_bits(x, prev)

    def split(self, x, bits, lds=None, offset=0):
        return split(x, bits)

    def bn_apply_split(self, z, scale, shift, relu, slope, bits, ldz=None):
        return split(bn_apply_value(z, scale, shift, relu, slope), bits)

    @staticmethod
    def _nt(a2, ba, bt2, bb, form, lda, bias):
        """a2 [M][K], bt2 [N][K] float32 at their pitched widths (K = taps * lda), K index tap-major"""
        (ah, al), (bh, bl) = plane_values(split(a2, ba)), plane_values(split(bt2, bb))
        acc = np.zeros((a2.shape[0], bt2.shape[0]), np.float32)
        kernel, _, taps, chunks = form[:4]
        if kernel == P.CONV:
            blocks = [slice(j * lda + 32 * cc, j * lda + 32 * cc + 32) for cc in range(chunks) for j in range(taps)]
        else:
            blocks = [slice(i, i + 16) for i in range(0, a2.shape[1], 16)]
        for s in blocks:
            for u, v in ((ah, bl), (al, bh), (ah, bh)):
                acc = acc + u[:, s] @ v[:, s].T
        out = acc * (np.float32(1) / (pow2_scale(ba) * pow2_scale(bb)))
        return out if bias is None else out + np.asarray(bias, np.float32)[None, :]

    def forward(self, x, kern, bias, stats=False, ldz=None, conv_wr=0):
        segs, t_in, c = x.shape
        k, _, o = kern.shape
        c_ld = P.align8(c)
        xp = np.zeros((segs, t_in, c_ld), np.float32)
        xp[:, :, :c] = x
        ax, aw = amax_bits(x), amax_bits(kern)
        form = P.nt_form(*P.forward_problem(segs, t_in, c_ld, k, o), stats=stats, conv_wr=conv_wr)
        z = f32(self._nt(spliced(xp, k), ax, weights_fwd(kern, c_ld), aw, form, c_ld, bias))
        return dict(z=z, part=f32(R.col_stats(z, np.float32)) if stats else None, ax=ax, aw=aw)

    def dgrad(self, dz, kern, bwd=None, conv_wr=0):
        segs, t_out, o = dz.shape
        k, c, _ = kern.shape
        o_ld = P.align8(o)
        dzp = np.zeros((segs, t_out + 2 * (k - 1), o_ld), np.float32)
        dzp[:, k - 1:k - 1 + t_out, :o] = dz
        adz, aw = amax_bits(dz), amax_bits(kern)
        form = P.nt_form(*P.dgrad_problem(segs, t_out, o_ld, k, c), bwd=bwd is not None, conv_wr=conv_wr)
        dx = f32(self._nt(spliced(dzp, k), adz, weights_dgrad(kern, o_ld), aw, form, o_ld, None))
        part = None if bwd is None else f32(bwd_partials(dx, bwd["z"], bwd["scale"], bwd["shift"], bwd["mean"], bwd["invstd"], np.float32))
        return dict(dx=dx, part=part, adz=adz, aw=aw)

    def wgrad(self, x, dz, kern, l2, pad=None):
        segs, t_in, c = x.shape
        k, _, o = kern.shape
        t_out = t_in - k + 1
        c_ld, o_ld = P.align8(c), P.align8(o)
        pad = k - 1 if pad is None else pad
        ax, adz = amax_bits(x), amax_bits(dz)
        plan = P.tn_plan(k * c_ld, o_ld, segs * t_out, t_out, t_in, t_out + 2 * pad)
        R_, r_chunk, splits = segs * t_out, plan[2], plan[1]

        def stages(v, cols):      # [splits][stages of a split][32 rows][cols] of both planes (the pad columns, all zero, left out); zero rows behind R (the kernel's zero page)
            planes = np.zeros((2, splits * r_chunk, cols), np.float32)
            planes[:, :R_] = split(v, amax_bits(v), cols).view(np.float16)
            return planes.reshape(2, splits, r_chunk // 32, 32, cols)

        a, b = stages(spliced(x, k), k * c), stages(dz.reshape(-1, o), o)
        acc = np.zeros((splits, k * c, o), np.float32)
        for st in range(r_chunk // 32):      # every split advances one stage: three products each, float32 accumulation
            for u, v in ((a[0], b[1]), (a[1], b[0]), (a[0], b[0])):
                acc = acc + np.matmul(u[:, st].transpose(0, 2, 1), v[:, st])
        scale = np.float32(1) / (pow2_scale(ax) * pow2_scale(adz))
        out = np.zeros((k * c, o), np.float32)
        for s in range(splits):
            out = out + acc[s] * scale
        dk = out.reshape(k, c, o)
        if l2 != 0:
            dk = dk + np.float32(l2) * np.asarray(kern, np.float32)
        return dict(dk=f32(dk), ax=ax, adz=adz)
