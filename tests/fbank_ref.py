"""fp64 / fp32 NumPy restatement of xv_fbank (include/xvector_hip.h): compute-fbank-feats with --dither=0, which is compute-mfcc-feats
stopped in front of the DCT.  Built on tests/mfcc_ref.py - the framing, the reflection, the pre-emphasis, the window and the mel triangles
are that module's functions, imported, not restated - and tied to it by tests/test_fbank_ref.py: the log-mel columns of this module times
mfcc_ref's DCT give mfcc_ref.mfcc.  Kaldi is not available where the tests run: parity BY RESTATEMENT, as there.  fbank(x, cfg, dtype) runs
every intermediate in `dtype`; float64 is the reference, float32 measures what the number format alone costs."""
import numpy as np

from tests import mfcc_ref as R

# compute-fbank-feats' own defaults
DEFAULTS = dict(sample_frequency=16000.0, frame_length_ms=25.0, frame_shift_ms=10.0, num_mel_bins=23, low_freq=20.0, high_freq=0.0, snip_edges=1,
                preemphasis=0.97, remove_dc_offset=1, use_energy=0, raw_energy=1, energy_floor=0.0, use_log_fbank=1, use_power=1)
EPS = R.EPS


def config(**kw):
    unknown = set(kw) - set(DEFAULTS)
    assert not unknown, unknown
    return dict(DEFAULTS, **kw)


def as_mfcc(cfg, **kw):
    """The mfcc_ref configuration with the fields the two programs share taken from cfg (num_ceps = num_mel_bins, no lifter unless kw says so)."""
    shared = {k: v for k, v in cfg.items() if k in R.DEFAULTS}
    return R.config(**dict(dict(shared, num_ceps=cfg["num_mel_bins"], cepstral_lifter=0.0), **kw))


def dims(cfg):
    return R.dims(cfg)


def num_frames(n, cfg):
    return R.num_frames(n, cfg)


def width(cfg):
    return cfg["num_mel_bins"] + (1 if cfg["use_energy"] else 0)


def tables(cfg):
    """mfcc_ref.tables without the dct."""
    t = R.tables(as_mfcc(cfg))
    del t["dct"]
    return t


def unpack_tables(flat, cfg):
    """The flat fp32 layout xv_fbank_tables writes: xv_mfcc_tables' without its last block."""
    L, S, N = dims(cfg)
    bins = cfg["num_mel_bins"]
    flat = np.asarray(flat, np.float32)
    at = 0
    window = flat[at:at + L]; at += L                           # noqa: E702
    twiddles = flat[at:at + N].reshape(N // 2, 2); at += N      # noqa: E702
    idx = flat[at:at + 3 * bins].reshape(bins, 3); at += 3 * bins      # noqa: E702
    first, count, off = (idx[:, j].astype(np.int64) for j in range(3))
    assert np.array_equal(idx, np.stack([first, count, off], axis=1).astype(np.float32)), "the index block holds whole numbers"
    assert np.array_equal(off, np.concatenate([[0], np.cumsum(count)[:-1]])), "weights are stored bin after bin"
    weights = [flat[at + off[m]:at + off[m] + count[m]] for m in range(bins)]
    at += int(count.sum())
    assert at == len(flat), (at, len(flat))
    return dict(window=window, twiddles=twiddles, mel_first=first, mel_count=count, mel_weights=weights)


def pack_tables(tb):
    """tables() in the flat layout, float64: one rounding to fp32 gives what xv_fbank_tables writes."""
    count = tb["mel_count"]
    off = np.concatenate([[0], np.cumsum(count)[:-1]])
    idx = np.stack([tb["mel_first"], count, off], axis=1).astype(np.float64)
    return np.concatenate([tb["window"], tb["twiddles"].reshape(-1), idx.reshape(-1)] + [np.asarray(w, np.float64) for w in tb["mel_weights"]])


def fbank(x, cfg, dtype=np.float64, with_energy=False):
    """x: n int16 samples -> [T, num_mel_bins + use_energy] in `dtype`, every intermediate in `dtype` (the tables rounded to it once);
    with_energy: (that, logE [T] of every frame, floored) - what xv_fbank hands to energy_out."""
    import scipy.fft
    dt = np.dtype(dtype).type
    L, S, N = dims(cfg)
    tb = tables(cfg)
    w = R.gather(x, cfg).astype(dtype)
    if w.shape[0] == 0:
        out = np.zeros((0, width(cfg)), dtype)
        return (out, np.zeros(0, dtype)) if with_energy else out
    eps = dt(EPS)
    if cfg["remove_dc_offset"]:
        w = w - w.sum(axis=1, keepdims=True, dtype=dtype) / dt(L)
    if cfg["raw_energy"]:
        log_e = np.log(np.maximum((w * w).sum(axis=1, dtype=dtype), eps))
    w = R.preemphasize(w, cfg["preemphasis"])
    w = w * tb["window"].astype(dtype)[None, :]
    if not cfg["raw_energy"]:
        log_e = np.log(np.maximum((w * w).sum(axis=1, dtype=dtype), eps))
    if cfg["energy_floor"] > 0:
        log_e = np.maximum(log_e, dt(np.log(cfg["energy_floor"])))
    X = scipy.fft.rfft(w, n=N, axis=1)
    assert X.dtype == (np.complex64 if dt is np.float32 else np.complex128)
    P = X.real * X.real + X.imag * X.imag
    if not cfg["use_power"]:
        P = np.sqrt(P)
    E = P[:, :N // 2] @ tb["mel_dense"].astype(dtype).T
    cols = np.log(np.maximum(E, eps)) if cfg["use_log_fbank"] else E
    out = np.concatenate([log_e[:, None], cols], axis=1) if cfg["use_energy"] else cols
    assert out.dtype == np.dtype(dtype) and log_e.dtype == np.dtype(dtype)
    return (out, log_e) if with_energy else out
