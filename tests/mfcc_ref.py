"""fp64 NumPy restatement of xv_mfcc and xv_energy_vad (include/xvector_hip.h): compute-mfcc-feats with --dither=0 and
compute-vad-decision, the two Kaldi programs behind steps/make_mfcc.sh and sid/compute_vad_decision.sh (egs/voxceleb/v1/run.sh:59-63).
Kaldi is not available where the tests run, so this is parity BY RESTATEMENT: the header states the rules, this module restates them, the
kernels are held against it.  The framing, reflection and pre-emphasis rules are written twice - vectorised for the GPU tests and as
literal per-sample loops (gather_loop, preemphasize_loop) - and tests/test_mfcc_ref.py holds one against the other.  mfcc(x, cfg, dtype)
runs every intermediate in `dtype`: float64 is the reference, float32 (scipy.fft.rfft keeps single precision) measures what the number
format alone costs - the GPU tests derive their tolerance from the distance between the two."""
import numpy as np

DEFAULTS = dict(sample_frequency=16000.0, frame_length_ms=25.0, frame_shift_ms=10.0, num_mel_bins=30, num_ceps=30, low_freq=20.0, high_freq=7600.0,
                snip_edges=0, preemphasis=0.97, remove_dc_offset=1, cepstral_lifter=22.0, use_energy=1, raw_energy=1, energy_floor=0.0)
VOXCELEB = dict(DEFAULTS)
SRE = dict(DEFAULTS, sample_frequency=8000.0, num_mel_bins=23, num_ceps=23, high_freq=3700.0)
THIRD = dict(DEFAULTS, use_energy=0, raw_energy=0, num_mel_bins=40, num_ceps=13, high_freq=-400.0, snip_edges=1)
CONFIGS = {"voxceleb": VOXCELEB, "sre": SRE, "third": THIRD}
VAD_VOXCELEB = dict(threshold=5.5, mean_scale=0.5, context=2, proportion=0.12)
EPS = float(np.finfo(np.float32).eps)      # FLT_EPSILON


def config(**kw):
    unknown = set(kw) - set(DEFAULTS)
    assert not unknown, unknown
    return dict(DEFAULTS, **kw)


def dims(cfg):
    """(L, S, N): samples per frame, per shift, FFT points."""
    L = int(cfg["sample_frequency"] * 0.001 * cfg["frame_length_ms"])
    S = int(cfg["sample_frequency"] * 0.001 * cfg["frame_shift_ms"])
    N = 1
    while N < L:
        N *= 2
    return L, S, N


def num_frames(n, cfg):
    L, S, _ = dims(cfg)
    if cfg["snip_edges"]:
        return 0 if n < L else 1 + (n - L) // S
    return (n + S // 2) // S


def gather(x, cfg):
    """x: n int16 samples -> [T, L] float64, frame f = the L samples from its first sample on, indices outside [0, n) reflected."""
    x = np.asarray(x)
    n = len(x)
    L, S, _ = dims(cfg)
    T = num_frames(n, cfg)
    if T == 0:
        return np.zeros((0, L))
    start = np.arange(T, dtype=np.int64) * S if cfg["snip_edges"] else S * np.arange(T, dtype=np.int64) + S // 2 - L // 2
    idx = start[:, None] + np.arange(L, dtype=np.int64)[None, :]
    while True:
        neg, over = idx < 0, idx >= n
        if not (neg.any() or over.any()):
            break
        idx = np.where(neg, -idx - 1, np.where(over, 2 * n - 1 - idx, idx))
    return x[idx].astype(np.float64)


def gather_loop(x, cfg):
    """The same, sample by sample, as the rule is stated."""
    n = len(x)
    L, S, _ = dims(cfg)
    T = num_frames(n, cfg)
    out = np.zeros((T, L))
    for f in range(T):
        first = f * S if cfg["snip_edges"] else S * f + S // 2 - L // 2
        for j in range(L):
            i = first + j
            while i < 0 or i >= n:
                i = -i - 1 if i < 0 else 2 * n - 1 - i
            out[f, j] = float(x[i])
    return out


def preemphasize(w, p):
    """[T, L] -> w[i] - p w[i - 1], the first sample minus p times itself; in w's dtype."""
    p = w.dtype.type(p)
    prev = np.concatenate([w[:, :1], w[:, :-1]], axis=1)
    return w - p * prev


def preemphasize_loop(w, p):
    """In place from the last sample down, as the rule is stated."""
    w = w.copy()
    p = w.dtype.type(p)
    for f in range(w.shape[0]):
        for i in range(w.shape[1] - 1, 0, -1):
            w[f, i] -= p * w[f, i - 1]
        w[f, 0] -= p * w[f, 0]
    return w


def mel(f):
    return 1127.0 * np.log(1.0 + np.asarray(f, np.float64) / 700.0)


def tables(cfg):
    """The constant tables in float64: window [L], twiddles [N/2, 2] = (cos, -sin)(2 pi k / N), mel_first / mel_count [bins], mel_weights (a
    list of bins arrays), mel_dense [bins, N/2] (the same weights as a matrix), dct [num_ceps, bins] with the lifter folded in."""
    L, S, N = dims(cfg)
    sf, bins, ceps = cfg["sample_frequency"], cfg["num_mel_bins"], cfg["num_ceps"]
    window = (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(L) / (L - 1))) ** 0.85
    k = np.arange(N // 2)
    twiddles = np.stack([np.cos(2.0 * np.pi * k / N), -np.sin(2.0 * np.pi * k / N)], axis=1)
    high = cfg["high_freq"] if cfg["high_freq"] > 0 else 0.5 * sf + cfg["high_freq"]
    mlo = float(mel(cfg["low_freq"]))
    delta = (float(mel(high)) - mlo) / (bins + 1)
    mk = mel(k * sf / N)
    dense = np.zeros((bins, N // 2))
    first, count, weights = [], [], []
    for m in range(bins):
        left, centre, right = mlo + m * delta, mlo + (m + 1) * delta, mlo + (m + 2) * delta
        inside = (mk > left) & (mk < right)
        w = np.where(mk <= centre, (mk - left) / (centre - left), (right - mk) / (right - centre))
        dense[m] = np.where(inside, w, 0.0)
        nz = np.flatnonzero(inside)
        first.append(int(nz[0]) if len(nz) else 0)
        count.append(int(nz[-1] - nz[0] + 1) if len(nz) else 0)
        weights.append(dense[m, first[-1]:first[-1] + count[-1]].copy())
    c = np.arange(ceps)[:, None]
    m = np.arange(bins)[None, :]
    dct = np.where(c == 0, np.sqrt(1.0 / bins), np.sqrt(2.0 / bins) * np.cos(np.pi / bins * (m + 0.5) * c))
    q = cfg["cepstral_lifter"]
    if q > 0:
        dct = dct * (1.0 + 0.5 * q * np.sin(np.pi * np.arange(ceps) / q))[:, None]
    return dict(window=window, twiddles=twiddles, mel_first=np.asarray(first), mel_count=np.asarray(count), mel_weights=weights, mel_dense=dense,
                dct=dct)


def unpack_tables(flat, cfg):
    """The flat fp32 layout xv_mfcc_tables writes (include/xvector_hip.h) -> the same dictionary (without mel_dense), fp32."""
    L, S, N = dims(cfg)
    bins, ceps = cfg["num_mel_bins"], cfg["num_ceps"]
    flat = np.asarray(flat, np.float32)
    at = 0
    window = flat[at:at + L]; at += L                           # noqa: E702
    twiddles = flat[at:at + N].reshape(N // 2, 2); at += N      # noqa: E702
    idx = flat[at:at + 3 * bins].reshape(bins, 3); at += 3 * bins      # noqa: E702
    first, count, off = (idx[:, j].astype(np.int64) for j in range(3))
    assert np.array_equal(idx, np.stack([first, count, off], axis=1).astype(np.float32)), "the index block holds whole numbers"
    n_w = int(count.sum())
    assert np.array_equal(off, np.concatenate([[0], np.cumsum(count)[:-1]])), "weights are stored bin after bin"
    weights = [flat[at + off[m]:at + off[m] + count[m]] for m in range(bins)]
    at += n_w
    dct = flat[at:at + ceps * bins].reshape(ceps, bins); at += ceps * bins      # noqa: E702
    assert at == len(flat), (at, len(flat))
    return dict(window=window, twiddles=twiddles, mel_first=first, mel_count=count, mel_weights=weights, dct=dct)


def mfcc(x, cfg, dtype=np.float64):
    """x: n int16 samples -> [T, num_ceps] in `dtype`, every intermediate in `dtype` (the tables rounded to it once)."""
    import scipy.fft
    dt = np.dtype(dtype).type
    L, S, N = dims(cfg)
    tb = tables(cfg)
    w = gather(x, cfg).astype(dtype)
    if w.shape[0] == 0:
        return np.zeros((0, cfg["num_ceps"]), dtype)
    eps = dt(EPS)
    if cfg["remove_dc_offset"]:
        w = w - w.sum(axis=1, keepdims=True, dtype=dtype) / dt(L)
    if cfg["raw_energy"]:
        log_e = np.log(np.maximum((w * w).sum(axis=1, dtype=dtype), eps))
    w = preemphasize(w, cfg["preemphasis"])
    w = w * tb["window"].astype(dtype)[None, :]
    if not cfg["raw_energy"]:
        log_e = np.log(np.maximum((w * w).sum(axis=1, dtype=dtype), eps))
    X = scipy.fft.rfft(w, n=N, axis=1)
    assert X.dtype == (np.complex64 if dt is np.float32 else np.complex128)
    P = X.real * X.real + X.imag * X.imag
    E = P[:, :N // 2] @ tb["mel_dense"].astype(dtype).T
    logmel = np.log(np.maximum(E, eps))
    c = logmel @ tb["dct"].astype(dtype).T
    if cfg["use_energy"]:
        if cfg["energy_floor"] > 0:
            log_e = np.maximum(log_e, dt(np.log(cfg["energy_floor"])))
        c[:, 0] = log_e
    assert c.dtype == np.dtype(dtype)
    return c


def vad_threshold(e, threshold, mean_scale):
    e = np.asarray(e, np.float64)
    return threshold + (mean_scale * (e.sum() / len(e)) if mean_scale != 0 and len(e) else 0.0)


def energy_vad(feats, threshold=5.5, mean_scale=0.5, context=2, proportion=0.12):
    """feats [T, d] (column 0 = the log-energy) -> uint8 [T]: frame t is voiced iff, of the frames of [t - context, t + context] inside
    [0, T), at least `proportion` (as fp32, the type it crosses the C-ABI in) of them lie above the threshold."""
    e = np.asarray(feats, np.float64)[:, 0]
    T = len(e)
    thr = vad_threshold(e, threshold, mean_scale)
    above = e > thr
    out = np.zeros(T, np.uint8)
    for t in range(T):
        lo, hi = max(t - context, 0), min(t + context, T - 1)
        out[t] = int(above[lo:hi + 1].sum()) >= (hi - lo + 1) * float(np.float32(proportion))
    return out


def signal(rs, n, sf):
    """The test signal: tones at 220, 1830 and 5200 Hz (amplitudes 3000, 1500, 800), every third quarter-second at 0.02 of that - a 40 dB
    dynamic range, so the VAD takes both decisions - plus Gaussian noise of sigma 40 and a DC offset of 37, rounded to int16."""
    t = np.arange(n) / float(sf)
    x = sum(a * np.sin(2.0 * np.pi * f * t) for f, a in ((220.0, 3000.0), (1830.0, 1500.0), (5200.0, 800.0)))
    x = x * np.where(np.floor(t / 0.25).astype(np.int64) % 3 == 2, 0.02, 1.0)
    x = x + rs.randn(n) * 40.0 + 37.0
    return np.rint(x).astype(np.int16)
