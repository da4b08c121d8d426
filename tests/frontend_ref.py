"""fp64 NumPy restatement of the extraction front end (xv_frontend, include/xvector_hip.h): Kaldi's SlidingWindowCmn with center = true and
normalize_variance = false (feat/feature-functions.cc), then select-voiced-frames, as egs/voxceleb/v1/nnet/run_extract_embeddings.sh:47
pipes them in front of extract.py.  Kaldi is not available where the tests run, so this is parity by restatement: the window rule is
written twice - vectorised here for the GPU tests, as a literal per-frame loop that sums each window directly (sliding_cmn_loop) - and
tests/test_frontend_ref.py holds one against the other."""
import numpy as np


def window_bounds(n, w):
    """[s, e) of every frame t of an n-frame utterance: s = t - w // 2, e = s + w, shifted back inside [0, n) and cut to it."""
    t = np.arange(n, dtype=np.int64)
    s = t - w // 2
    e = s + w
    neg = s < 0
    e = np.where(neg, e - s, e)
    s = np.where(neg, 0, s)
    over = e > n
    s = np.where(over, np.maximum(s - (e - n), 0), s)
    e = np.where(over, n, e)
    return s, e


def sliding_cmn(x, w):
    """x [n, d] -> x - (mean of its window) in float64; w = 0: x itself.  Window sums are differences of a prefix sum carried in
    extended precision (np.longdouble), so their error is far below one float64 rounding of the mean."""
    x = np.asarray(x, np.float64)
    if w <= 0:
        return x.copy()
    n = x.shape[0]
    s, e = window_bounds(n, w)
    prefix = np.zeros((n + 1, x.shape[1]), np.longdouble)
    np.cumsum(x.astype(np.longdouble), axis=0, out=prefix[1:])
    mean = ((prefix[e] - prefix[s]) / (e - s)[:, None].astype(np.longdouble)).astype(np.float64)
    return x - mean


def sliding_cmn_loop(x, w):
    """The same, frame by frame, every window summed directly (the rule as the issue and Kaldi's loop state it)."""
    x = np.asarray(x, np.float64)
    n = x.shape[0]
    out = np.empty_like(x)
    for t in range(n):
        s = t - w // 2
        e = s + w
        if s < 0:
            e -= s
            s = 0
        if e > n:
            s -= e - n
            e = n
            s = max(s, 0)
        out[t] = x[t] - x[s:e].sum(axis=0) / (e - s)
    return out


def frontend(x, w=0, mask=None, first=0, count=None):
    """One piece: CMN over the RAW utterance, then rows [first, first + count) of its voiced frames (mask None: all).  float64 [rows, d]."""
    y = sliding_cmn(x, w)
    if mask is not None:
        y = y[np.flatnonzero(np.asarray(mask) != 0)]
    y = y[first:]
    return y if count is None else y[:count]


def raw_features(rs, n, d):
    """MFCC-like test input: randn * 20 + 50, column 0 shifted by -120."""
    x = rs.randn(n, d) * 20 + 50
    x[:, 0] -= 120
    return x.astype(np.float32)
