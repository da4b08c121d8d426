"""NumPy restatement of xv_augment (include/xvector_hip.h, steps 1 - 7): wav-reverberate with --normalize-output=true as this project
restates it.  Kaldi is not available where the tests run, so this is parity BY RESTATEMENT: the header states the rules, this module
restates them, the kernels are held against it.  augment(..., dtype=np.float64) is the reference: every sum of the convolution is a whole
number below 2^53, so it is exact up to the scale factors.  dtype=np.float32 follows the kernels' number format - taps in blocks of `kb`
anchored at tap 0, a block summed sequentially from zero with one fma per tap, the block sums added sequentially, every power in double,
the gains and the scale rounded to fp32 once - and measures what the format alone costs: the GPU tests derive their tolerance from the
distance between the two.  An fma of fp32 values is formed in double (the product of an fp32 and an int16-valued float is exact there)
and rounded once."""
import numpy as np


def early(h, fs=16000.0):
    """(es, ee, p): the first index of the maximum and the early part around it, the products in fp32, truncated."""
    h = np.asarray(h)
    p = int(np.argmax(h))
    return max(p - int(np.float32(0.001) * np.float32(fs)), 0), min(p + int(np.float32(0.05) * np.float32(fs)), len(h)), p


def _fma32(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def conv64(x, h):
    return np.convolve(np.asarray(x, np.float64), np.asarray(h, np.float64))


def conv32(x, h, kb):
    """The full convolution in fp32 with the kernels' add chain: kb + ceil(L / kb) roundings at most per output."""
    x, h = np.asarray(x, np.float32), np.asarray(h, np.float32)
    n, L = len(x), len(h)
    acc = np.zeros(n + L - 1, np.float32)
    for k0 in range(0, L, kb):
        blk = np.zeros(n + L - 1, np.float32)
        for k in range(k0, min(k0 + kb, L)):
            blk[k:k + n] = _fma32(h[k], x, blk[k:k + n])
        acc = acc + blk
    return acc


def noise_signal(v, span):
    """v[i mod len] for i < span."""
    v = np.asarray(v)
    return v[np.arange(span, dtype=np.int64) % len(v)]


def quantise(v):
    """Step 7: truncate toward zero, then clamp -> (int16, how many samples the clamp changed)."""
    t = np.trunc(np.asarray(v, np.float64))
    c = np.clip(t, -32768.0, 32767.0)
    return c.astype(np.int16), int((c != t).sum())


def _conv(x, h, f32, kb, cache):
    """conv32 / conv64 through `cache` (a dict, or None): a test that runs one utterance under several configurations convolves once."""
    if cache is None:
        return conv32(x, h, kb) if f32 else conv64(x, h)
    key = (x.tobytes(), h.tobytes(), f32, kb if f32 else 0)
    if key not in cache:
        cache[key] = conv32(x, h, kb) if f32 else conv64(x, h)
        cache[key].setflags(write=False)
    return cache[key].copy()


def augment(x, h=None, noises=(), fs=16000.0, shift_output=1, normalize_output=1, volume=0.0, dtype=np.float64, kb=32, details=None, cache=None):
    """x, h: int16 arrays (h None: no impulse response); noises: (v int16, snr dB, start sample, span | None = len(v), a foreground noise |
    "bg" = M) in list order -> the n_out samples of step 6 in `dtype` (not quantised).  details: a dict that receives P0, E, gains, scale,
    M, p and the magnitude sum |x| * |h| + sum g_j |v_j| in the order of the output (the derived bound's)."""
    f32 = dtype == np.float32
    x = np.asarray(x)
    n = len(x)
    xd = x.astype(np.float64)
    P0 = float((xd * xd).sum() / n)
    if h is not None:
        h = np.asarray(h)
        es, ee, p = early(h, fs)
        e = _conv(x, h[es:ee], f32, kb, cache).astype(np.float64)
        assert len(e) == n + (ee - es) - 1
        E = float((e * e).sum() / len(e))
        y = _conv(x, h, f32, kb, cache)
        mag = np.convolve(np.abs(xd), np.abs(h.astype(np.float64)))
    else:
        E, p = P0, 0
        y = x.astype(dtype)
        mag = np.abs(xd)
    M = len(y)
    gains = []
    for v, snr, start, span in noises:
        v = np.asarray(v)
        span = len(v) if span is None else M if span == "bg" else int(span)
        s = noise_signal(v, span).astype(np.float64)
        Pn = float((s * s).sum() / span)
        if Pn == 0.0 or start >= M:
            gains.append(0.0)
            continue
        g = np.sqrt(np.power(10.0, -float(np.float32(snr)) / 10.0) * E / Pn)
        g = np.float32(g) if f32 else g
        gains.append(float(g))
        m = min(span, M - start)
        y[start:start + m] = _fma32(g, s[:m], y[start:start + m]) if f32 else y[start:start + m] + g * s[:m]
        mag[start:start + m] += float(g) * np.abs(s[:m])
    yd = y.astype(np.float64)
    Pa = float((yd * yd).sum() / M)
    scale = (np.sqrt(P0 / Pa) if normalize_output and Pa > 0.0 else 1.0) * (float(np.float32(volume)) if volume > 0 else 1.0)
    scale = np.float32(scale) if f32 else scale
    y = y * scale
    assert y.dtype == dtype
    shift, n_out = (p, n) if shift_output else (0, M)
    idx = (np.arange(n_out, dtype=np.int64) + shift) % M
    if details is not None:
        details.update(P0=P0, E=E, gains=gains, scale=float(scale), M=M, p=p, Pa=Pa, magnitude=mag[idx])
    return y[idx]


def signal(rs, n):
    """n int16 samples, |x| <= 8000: two tones under a slow envelope plus noise."""
    t = np.arange(n, dtype=np.float64) / 16000.0
    f1, f2 = rs.uniform(150.0, 400.0), rs.uniform(900.0, 3000.0)
    env = 0.55 + 0.45 * np.sin(2 * np.pi * rs.uniform(1.0, 4.0) * t + rs.uniform(0, 6.28))
    x = env * (3000.0 * np.sin(2 * np.pi * f1 * t + rs.uniform(0, 6.28)) + 2000.0 * np.sin(2 * np.pi * f2 * t)) + 600.0 * rs.randn(n)
    x = np.clip(np.round(x), -8000, 8000).astype(np.int16)
    if not x.any():
        x[0] = 1000
    return x


def rir(rs, L, peak):
    """L int16 taps: about 29 000 at `peak` (the one maximum), small taps in front, a decaying tail of either sign behind, h[0] != 0 and
    |h[L - 1]| >= 1500 - a dropped first or last tap moves outputs by far more than any tolerance."""
    assert 0 <= peak < L
    i = np.arange(L, dtype=np.float64)
    sign = np.where(rs.rand(L) < 0.5, -1.0, 1.0)
    tail = 12000.0 * np.exp(-(i - peak) / max(L / 3.0, 1.0)) * rs.uniform(0.3, 1.0, L)
    h = np.where(i > peak, tail, rs.uniform(200.0, 2000.0, L)) * sign
    h[peak] = 29000.0 + rs.randint(0, 200)
    if peak != L - 1 and abs(h[L - 1]) < 1500.0:
        h[L - 1] = 1500.0 * sign[L - 1] * rs.uniform(1.0, 1.5)
    h = np.round(h).astype(np.int16)
    assert h[0] != 0 and abs(int(h[L - 1])) >= 1500 and int(np.argmax(h)) == peak and (np.delete(h, peak) < 29000).all()
    return h
