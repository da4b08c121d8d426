"""Op-level Python wrappers over the C-ABI (include/xvector_hip.h, "Op level").

Inputs/outputs are torch CUDA tensors used purely as device buffers; every
function enqueues HIP kernels on torch's current stream.  No arithmetic is done
by torch here.  These are what the per-kernel parity tests call.
"""
import ctypes as C

import torch

try:
    from . import _lib
except ImportError:
    import _lib

TILE_M = 128


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _s():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _f32(shape, like):
    return torch.empty(shape, dtype=torch.float32, device=like.device)


_WS = {}


def workspace(device, nbytes=256 << 20):
    key = (str(device), nbytes)
    if key not in _WS:
        _WS[key] = torch.empty(nbytes // 4, dtype=torch.float32, device=device)
    return _WS[key]


def _ws(t):
    w = workspace(t.device)
    return _p(w), C.c_size_t(w.numel() * 4)


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


def frontend(x, rows_in, cmn_window=0, masks=None, mask_offsets=None, first=None, count=None, t_out=None):
    """Sliding-window CMN (cmn_window frames, 0 = off), then voiced-frame selection, on a decoded batch x [b, t_in, d] with rows_in[i] raw
    frames per piece (xv_frontend).  masks: uint8 device tensor, the pieces' voicing masks back to back, piece i's at byte
    mask_offsets[i] (int64) - None keeps every frame; first / count (int32, None = 0 / t_out): the range of SELECTED rows a piece
    keeps.  -> (out [b, t_out, d], rows_out int32 [b])."""
    b, t_in, d = x.shape
    t_out = t_in if t_out is None else int(t_out)
    out = torch.empty((b, t_out, d), dtype=torch.float32, device=x.device)
    rows_out = torch.empty(b, dtype=torch.int32, device=x.device)
    ws = torch.empty((b, t_out), dtype=torch.int32, device=x.device) if masks is not None else None
    _lib.call("xv_frontend", _s(), _p(x), _p(rows_in), b, t_in, d, int(cmn_window), _p(masks), C.c_size_t(masks.numel() if masks is not None else 0),
              _p(mask_offsets), _p(first), _p(count), t_out, _p(out), _p(rows_out), _p(ws), C.c_size_t(ws.numel() * 4 if ws is not None else 0))
    return out, rows_out


def mfcc_config(**kw):
    """xv_mfcc_config with the VoxCeleb conf/mfcc.conf defaults (dither 0); keyword arguments name the fields to change."""
    return _lib.XvMfccConfig(**kw)


def mfcc_num_frames(cfg, samples):
    n = int(_lib.load().xv_mfcc_num_frames(C.byref(cfg), C.c_int64(int(samples))))
    if n < 0:
        _lib.check(2, "xv_mfcc_num_frames")
    return n


def mfcc_tables(cfg):
    """The constant tables of xv_mfcc for cfg as a host float32 array (xv_mfcc_tables: host arithmetic, no GPU call)."""
    import numpy as np
    lib = _lib.load()
    n = int(lib.xv_mfcc_table_floats(C.byref(cfg)))
    if n == 0:
        _lib.check(2, "xv_mfcc_table_floats")
    flat = np.empty(n, np.float32)
    _lib.check(lib.xv_mfcc_tables(C.byref(cfg), C.c_void_p(flat.ctypes.data), C.c_size_t(n)), "xv_mfcc_tables")
    return flat


def mfcc(cfg, tables, pcm, offsets, samples, t_out=None):
    """MFCCs of a batch of waveforms (xv_mfcc).  tables: mfcc_tables(cfg) on the device; pcm: int16 device tensor, the utterances back to back;
    offsets / samples: HOST integer arrays [b] - utterance i is pcm[offsets[i] : offsets[i] + samples[i]] (the kernel does not check them, so
    they are checked here, before the upload).  t_out: rows of the output (default: the longest frame count).
    -> (out [b, t_out, num_ceps] float32, rows_out int32 [b] = min(frames, t_out); rows behind are zero)."""
    import numpy as np
    if pcm.dtype != torch.int16 or pcm.dim() != 1 or not pcm.is_contiguous():
        raise ValueError("mfcc: pcm must be a contiguous 1-D int16 tensor")
    offsets, samples = np.asarray(offsets), np.asarray(samples)
    if offsets.ndim != 1 or offsets.shape != samples.shape or offsets.size == 0 or offsets.dtype.kind not in "iu" or samples.dtype.kind not in "iu":
        raise ValueError("mfcc: offsets and samples must be two non-empty 1-D integer arrays of one length")
    if offsets.min() < 0 or samples.min() < 0 or (offsets.astype(np.int64) + samples.astype(np.int64)).max() > pcm.numel():
        raise IndexError("mfcc: an utterance lies outside the %d samples of pcm" % pcm.numel())
    if samples.max() >= 2 ** 31:
        raise ValueError("mfcc: an utterance holds 2^31 samples or more")
    if tables.dtype != torch.float32 or not tables.is_contiguous() or tables.numel() != int(_lib.load().xv_mfcc_table_floats(C.byref(cfg))):
        raise ValueError("mfcc: tables must be mfcc_tables(cfg) as a contiguous float32 device tensor")
    b = offsets.size
    if t_out is None:
        t_out = max(max(mfcc_num_frames(cfg, n) for n in samples), 1)
    t_out = int(t_out)
    off_d = torch.from_numpy(np.ascontiguousarray(offsets, dtype=np.int64)).to(pcm.device)
    n_d = torch.from_numpy(np.ascontiguousarray(samples, dtype=np.int32)).to(pcm.device)
    out = torch.empty((b, t_out, int(cfg.num_ceps)), dtype=torch.float32, device=pcm.device)
    rows_out = torch.empty(b, dtype=torch.int32, device=pcm.device)
    _lib.call("xv_mfcc", _s(), C.byref(cfg), _p(tables), _p(pcm), _p(off_d), _p(n_d), b, t_out, _p(out), _p(rows_out))
    return out, rows_out


def energy_vad(x, rows, threshold=5.5, mean_scale=0.5, frames_context=2, proportion=0.12):
    """compute-vad-decision on a padded batch x [b, t, d] with rows[i] (int32 device tensor) frames per piece (xv_energy_vad; the defaults
    are the VoxCeleb vad.conf) -> uint8 [b, t], 1 = voiced, bytes behind rows[i] zero: the masks ops.frontend reads with
    mask_offsets[i] = i * t."""
    if x.dim() != 3 or x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError("energy_vad: x must be a contiguous float32 [b, t, d] tensor")
    if rows.dtype != torch.int32 or rows.numel() != x.shape[0]:
        raise ValueError("energy_vad: rows must hold one int32 per piece")
    b, t, d = x.shape
    masks = torch.empty((b, t), dtype=torch.uint8, device=x.device)
    _lib.call("xv_energy_vad", _s(), _p(x), _p(rows), b, t, d, C.c_float(threshold), C.c_float(mean_scale), int(frames_context),
              C.c_float(proportion), _p(masks))
    return masks


def augment_config(**kw):
    """xv_augment_config with wav-reverberate's recipe settings (16 kHz, shift_output, normalize_output, no volume); keyword arguments
    name the fields to change."""
    return _lib.XvAugmentConfig(**kw)


def augment_plan(n, taps=0):
    """xv_debug_augment_plan: {tiles, tile, kb, chain} of an utterance of n samples under `taps` taps (0: no impulse response)."""
    out = (C.c_int * 4)()
    _lib.check(_lib.load().xv_debug_augment_plan(C.c_int64(int(n)), C.c_int64(int(taps)), out), "xv_debug_augment_plan")
    return dict(tiles=out[0], tile=out[1], kb=out[2], chain=out[3])


def augment_workspace_bytes(b, n_entries, n_tiles):
    return int(_lib.load().xv_augment_workspace_bytes(int(b), int(n_entries), C.c_int64(int(n_tiles))))


def augment_early(h, sample_frequency):
    """(es, ee, p) of an impulse response (host array): p the first index of its maximum, the early part h[es:ee] from 1 ms in front of
    the peak to 50 ms behind it, the products taken in fp32 and truncated (include/xvector_hip.h, step 2)."""
    import numpy as np
    h = np.asarray(h).reshape(-1)
    if h.size == 0:
        raise ValueError("augment_early: an impulse response needs at least one tap")
    p, fs = int(np.argmax(h)), np.float32(sample_frequency)
    return max(p - int(np.float32(0.001) * fs), 0), min(p + int(np.float32(0.05) * fs), h.size), p


def _aug_ints(a, what, n=None):
    import numpy as np
    a = np.asarray(a)
    if a.ndim != 1 or a.dtype.kind not in "iu" or (n is not None and a.size != n):
        raise ValueError("augment: %s must be a 1-D integer array%s" % (what, "" if n is None else " of %d" % n))
    return a.astype(np.int64)


def _aug_pool(t, what):
    if t is None:
        return 0
    if t.dtype != torch.int16 or t.dim() != 1 or not t.is_contiguous():
        raise ValueError("augment: %s must be a contiguous 1-D int16 tensor" % what)
    return t.numel()


def augment(cfg, src, src_off, src_len, rir=None, rir_off=None, rir_len=None, rir_early=None, utt_rir=None, noise=None, noise_off=None,
            noise_len=None, nz_first=None, nz_id=None, nz_snr=None, nz_start=None, nz_span=None, out_offsets=None, out_pcm=None,
            out_f32=False):
    """Reverberation and additive noise on a batch of waveforms (xv_augment; include/xvector_hip.h states the arithmetic).
    src / rir / noise: int16 device tensors, the pools' signals back to back; every other argument is a HOST array, checked here before
    the one upload (the kernels check nothing).  Utterance i is src[src_off[i] : src_off[i] + src_len[i]]; utt_rir[i] names its impulse
    response (-1 or utt_rir=None: none), rir k being rir[rir_off[k] : rir_off[k] + rir_len[k]] with rir_early[k] = augment_early(...) =
    (es, ee, p); its noises are the entries nz_first[i] .. nz_first[i + 1] (CSR, [b + 1]) in list order: noise nz_id[e] at nz_snr[e] dB
    from sample nz_start[e] over nz_span[e] samples (-1: the background form, the utterance's M).  out_offsets (default: back to back) /
    out_pcm (default: a new tensor that just holds them): where the outputs go; out_f32: True for a new float32 tensor of out_pcm's
    size, or such a tensor.  -> (out_pcm int16, out_offsets int64 host array, out_samples int32 [b], clipped int32 [b], out_f32 | None)."""
    import numpy as np
    n_src, n_rir_pool, n_noise_pool = _aug_pool(src, "src"), _aug_pool(rir, "rir"), _aug_pool(noise, "noise")
    src_off, src_len = _aug_ints(src_off, "src_off"), _aug_ints(src_len, "src_len")
    b = src_off.size
    if b == 0 or src_len.size != b:
        raise ValueError("augment: src_off and src_len must be two non-empty arrays of one length")
    if src_off.min() < 0 or src_len.min() < 1 or (src_off + src_len).max() > n_src:
        raise IndexError("augment: a source is empty or lies outside the %d samples of src" % n_src)
    utt_rir = np.full(b, -1, np.int64) if utt_rir is None else _aug_ints(utt_rir, "utt_rir", b)
    any_rir = bool((utt_rir >= 0).any())
    taps = np.zeros(b, np.int64)
    rir_words = np.zeros((b, 5), np.int64)
    rir_words[:, 0] = -1
    if any_rir:
        rir_off, rir_len = _aug_ints(rir_off, "rir_off"), _aug_ints(rir_len, "rir_len", np.asarray(rir_off).size)
        early = np.asarray(rir_early, dtype=np.int64).reshape(-1, 3)
        if early.shape[0] != rir_off.size:
            raise ValueError("augment: rir_early must hold (es, ee, p) of each of the %d impulse responses" % rir_off.size)
        if rir_off.size == 0 or rir_off.min() < 0 or rir_len.min() < 1 or (rir_off + rir_len).max() > n_rir_pool:
            raise IndexError("augment: an impulse response is empty or lies outside the %d samples of rir" % n_rir_pool)
        if (early[:, 0] < 0).any() or (early[:, 0] >= early[:, 1]).any() or (early[:, 1] > rir_len).any() or (early[:, 2] < 0).any() \
                or (early[:, 2] >= rir_len).any():
            raise ValueError("augment: rir_early must satisfy 0 <= es < ee <= L and 0 <= p < L")
        if utt_rir.max() >= rir_off.size or utt_rir.min() < -1:
            raise IndexError("augment: utt_rir names an impulse response outside 0 .. %d" % (rir_off.size - 1))
        has = utt_rir >= 0
        k = utt_rir[has]
        taps[has] = rir_len[k]
        rir_words[has] = np.stack([rir_off[k], rir_len[k], early[k, 0], early[k, 1], early[k, 2]], axis=1)
    m_len = np.where(taps > 0, src_len + taps - 1, src_len)
    if m_len.max() >= 2 ** 31:
        raise ValueError("augment: an utterance would hold 2^31 samples or more")
    nz_first = np.zeros(b + 1, np.int64) if nz_first is None else _aug_ints(nz_first, "nz_first", b + 1)
    n_entries = int(nz_first[-1])
    if nz_first[0] != 0 or (np.diff(nz_first) < 0).any():
        raise ValueError("augment: nz_first must rise from 0 (CSR)")
    noise_words = np.zeros((n_entries, 5), np.int64)
    if n_entries:
        noise_off, noise_len = _aug_ints(noise_off, "noise_off"), _aug_ints(noise_len, "noise_len", np.asarray(noise_off).size)
        if noise_off.size == 0 or noise_off.min() < 0 or noise_len.min() < 1 or (noise_off + noise_len).max() > n_noise_pool:
            raise IndexError("augment: a noise is empty or lies outside the %d samples of noise" % n_noise_pool)
        nz_id, nz_start, nz_span = _aug_ints(nz_id, "nz_id", n_entries), _aug_ints(nz_start, "nz_start", n_entries), _aug_ints(nz_span, "nz_span", n_entries)
        snr = np.asarray(nz_snr, dtype=np.float32).reshape(-1)
        if snr.size != n_entries or not np.isfinite(snr).all() or np.abs(snr).max() > 200:
            raise ValueError("augment: nz_snr must hold one finite SNR within +-200 dB per noise entry")
        if nz_id.min() < 0 or nz_id.max() >= noise_off.size:
            raise IndexError("augment: nz_id names a noise outside 0 .. %d" % (noise_off.size - 1))
        owner = np.repeat(np.arange(b), np.diff(nz_first))
        nz_span = np.where(nz_span == -1, m_len[owner], nz_span)
        if nz_start.min() < 0 or nz_span.min() < 1 or nz_start.max() >= 2 ** 31 or nz_span.max() >= 2 ** 31:
            raise ValueError("augment: nz_start must lie in 0 .. 2^31 and nz_span in 1 .. 2^31 (or be -1: the background form)")
        noise_words = np.stack([noise_off[nz_id], noise_len[nz_id], snr.view(np.uint32).astype(np.int64), nz_start, nz_span], axis=1)
    n_out = src_len if cfg.shift_output else m_len
    if out_offsets is None:
        out_offsets = np.concatenate([[0], np.cumsum(n_out)[:-1]]).astype(np.int64)
    out_offsets = _aug_ints(out_offsets, "out_offsets", b)
    if out_pcm is None:
        out_pcm = torch.empty(int((out_offsets + n_out).max()), dtype=torch.int16, device=src.device)
    total = _aug_pool(out_pcm, "out_pcm")
    order = np.argsort(out_offsets, kind="stable")
    if out_offsets.min() < 0 or (out_offsets + n_out).max() > total or (out_offsets[order][1:] < (out_offsets + n_out)[order][:-1]).any():
        raise IndexError("augment: the outputs overlap or lie outside the %d samples of out_pcm" % total)
    if out_f32 is True:
        out_f32 = torch.empty(total, dtype=torch.float32, device=src.device)
    elif out_f32 is False:
        out_f32 = None
    elif out_f32.dtype != torch.float32 or out_f32.dim() != 1 or not out_f32.is_contiguous() or out_f32.numel() < total:
        raise ValueError("augment: out_f32 must be a contiguous 1-D float32 tensor of out_pcm's size")
    tile = augment_plan(1)["tile"]
    tiles = (m_len + tile - 1) // tile
    n_tiles = int(tiles.sum())
    tile_utt = np.repeat(np.arange(b, dtype=np.int64), tiles)
    tile_first = (np.arange(n_tiles, dtype=np.int64) - np.repeat(np.cumsum(tiles) - tiles, tiles)) * tile
    utt_words = np.concatenate([np.stack([src_off, src_len], axis=1), rir_words, np.stack([nz_first[:-1], np.diff(nz_first), out_offsets], axis=1)], axis=1)
    assert utt_words.shape == (b, _lib.XV_AUG_UTT_WORDS) and noise_words.shape == (n_entries, _lib.XV_AUG_NOISE_WORDS)
    tables = np.concatenate([utt_words.reshape(-1), noise_words.reshape(-1), np.stack([tile_utt, tile_first], axis=1).reshape(-1)]).astype(np.int64)
    tables_d = torch.from_numpy(np.ascontiguousarray(tables)).to(src.device)
    ws_bytes = augment_workspace_bytes(b, n_entries, n_tiles)
    ws = torch.empty((ws_bytes + 7) // 8, dtype=torch.float64, device=src.device)
    out_samples = torch.empty(b, dtype=torch.int32, device=src.device)
    clipped = torch.empty(b, dtype=torch.int32, device=src.device)
    _lib.call("xv_augment", _s(), C.byref(cfg), b, n_entries, C.c_int64(n_tiles), _p(src), _p(rir), _p(noise), _p(tables_d), C.c_size_t(tables.size),
              int(any_rir), _p(ws), C.c_size_t(ws_bytes), _p(out_pcm), _p(out_f32), _p(out_samples), _p(clipped))
    return out_pcm, out_offsets, out_samples, clipped, out_f32


def _pitched(t, what):
    """(rows, pitch in floats) of a 2-D float32 device view with contiguous rows."""
    if t.dim() != 2 or t.dtype != torch.float32 or (t.shape[1] > 1 and t.stride(1) != 1):
        raise ValueError("%s: a 2-D float32 tensor with contiguous rows is expected" % what)
    return t.shape[0], t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1])


def score_prepare(x, d=None, mean=None, out=None):
    """Rows of x [rows, >= d] minus mean [d] (None: nothing subtracted), scaled to unit length (xv_score_prepare).  d: the columns that
    hold the vector (default: all of x).  out: the [rows, ldy] tensor to write (may be x itself, in place); default a new tensor whose
    pitch is d rounded up to 4 - columns d .. ldy come back zero, so the result is a GEMM operand for score_cohort_stats."""
    rows, ldx = _pitched(x, "score_prepare: x")
    d = x.shape[1] if d is None else int(d)
    if out is None:
        out = torch.empty((rows, (d + 3) // 4 * 4), dtype=torch.float32, device=x.device)
    _, ldy = _pitched(out, "score_prepare: out")
    if out.shape[1] != ldy:
        raise ValueError("score_prepare: out must be the whole [rows, pitch] buffer (its padding columns are written)")
    if mean is not None and (mean.dtype != torch.float32 or mean.numel() != d or not mean.is_contiguous()):
        raise ValueError("score_prepare: mean must be %d contiguous float32 values" % d)
    _lib.call("xv_score_prepare", _s(), _p(x), rows, d, ldx, _p(mean), _p(out), ldy)
    return out


def score_trials(e, t, d, ei, ti, e_stats=None, t_stats=None):
    """out[j] = e[ei[j]][:d] . t[ti[j]][:d], AS-normalised with the rows' cohort statistics when both are given (xv_score_trials).
    ei, ti: HOST integer arrays (NumPy / sequences): the kernel does not check indices, so they are checked here, before the upload."""
    import numpy as np
    ne, lde = _pitched(e, "score_trials: e")
    nt, ldt = _pitched(t, "score_trials: t")
    ei, ti = np.asarray(ei), np.asarray(ti)
    if ei.ndim != 1 or ei.shape != ti.shape or ei.size == 0 or ei.dtype.kind not in "iu" or ti.dtype.kind not in "iu":
        raise ValueError("score_trials: ei and ti must be two non-empty 1-D integer arrays of one length")
    if ei.min() < 0 or ei.max() >= ne:
        raise IndexError("score_trials: ei holds an index outside 0 .. %d" % (ne - 1))
    if ti.min() < 0 or ti.max() >= nt:
        raise IndexError("score_trials: ti holds an index outside 0 .. %d" % (nt - 1))
    for st, n, name in ((e_stats, ne, "e_stats"), (t_stats, nt, "t_stats")):
        if st is not None and (st.dtype != torch.float32 or tuple(st.shape) != (n, 2) or not st.is_contiguous()):
            raise ValueError("score_trials: %s must be a contiguous float32 [%d, 2] tensor" % (name, n))
    ei_d = torch.from_numpy(np.ascontiguousarray(ei, dtype=np.int32)).to(e.device)
    ti_d = torch.from_numpy(np.ascontiguousarray(ti, dtype=np.int32)).to(e.device)
    out = torch.empty(ei.size, dtype=torch.float32, device=e.device)
    _lib.call("xv_score_trials", _s(), _p(e), lde, ne, _p(t), ldt, nt, int(d), _p(ei_d), _p(ti_d), C.c_int64(ei.size), _p(e_stats), _p(t_stats),
              _p(out))
    return out


def score_cohort_workspace_bytes(rows, n_cohort, d):
    return int(_lib.load().xv_score_cohort_workspace_bytes(int(rows), int(n_cohort), int(d)))


def score_cohort_stats(x, cohort, d, top_k, ws_bytes=None):
    """[rows, 2] = (mean, biased deviation) of each row's min(top_k, n_cohort) largest scores against the cohort rows
    (xv_score_cohort_stats).  x, cohort: prepared matrices (score_prepare: zero padding up to a pitch that is a multiple of 4).
    ws_bytes: size of the score slab (default: the whole call in one GEMM launch); fewer bytes run the rows in tiles."""
    rows, ldx = _pitched(x, "score_cohort_stats: x")
    n_cohort, ldc = _pitched(cohort, "score_cohort_stats: cohort")
    if ws_bytes is None:
        ws_bytes = score_cohort_workspace_bytes(rows, n_cohort, d)
    ws = torch.empty(max(int(ws_bytes) // 4, 1), dtype=torch.float32, device=x.device)
    stats = torch.empty((rows, 2), dtype=torch.float32, device=x.device)
    _lib.call("xv_score_cohort_stats", _s(), _p(x), ldx, rows, _p(cohort), ldc, n_cohort, int(d), int(top_k), _p(stats), _p(ws),
              C.c_size_t(int(ws_bytes)))
    return stats


def _host_int(a, what, lo, hi):
    """A 1-D host integer array with every value in [lo, hi), as a contiguous NumPy array (its dtype unchanged)."""
    import numpy as np
    a = np.asarray(a)
    if a.ndim != 1 or a.size == 0 or a.dtype.kind not in "iu":
        raise ValueError("%s must be a non-empty 1-D integer array" % what)
    if a.min() < lo or a.max() >= hi:
        raise IndexError("%s holds a value outside %d .. %d" % (what, lo, hi - 1))
    return a


def backend_group_means(x, d, offsets, rows, want32=True):
    """Averages of groups of rows of x [n, >= d] (xv_backend_group_means): group g = rows[offsets[g]:offsets[g + 1]], added in list order in
    double.  offsets, rows: HOST integer arrays (the kernel does not check them, so they are checked here: an empty group and a row outside
    x are refused).  -> (mean64 [groups, d] float64, mean32 [groups, d rounded up to 4] float32 with zero padding, or None)."""
    import numpy as np
    n, ldx = _pitched(x, "backend_group_means: x")
    offsets = np.asarray(offsets)
    if offsets.ndim != 1 or offsets.size < 2 or offsets.dtype.kind not in "iu" or offsets[0] != 0:
        raise ValueError("backend_group_means: offsets must be a 1-D integer array [groups + 1] that starts at 0")
    counts = np.diff(offsets.astype(np.int64))
    if counts.min() <= 0:
        raise ValueError("backend_group_means: group %d is empty" % int(np.argmax(counts <= 0)))
    rows = _host_int(rows, "backend_group_means: rows", 0, n)
    if rows.size != int(offsets[-1]):
        raise ValueError("backend_group_means: offsets end at %d, rows holds %d indices" % (int(offsets[-1]), rows.size))
    groups = offsets.size - 1
    off_d = torch.from_numpy(np.ascontiguousarray(offsets, dtype=np.int64)).to(x.device)
    rows_d = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int32)).to(x.device)
    mean64 = torch.empty((groups, int(d)), dtype=torch.float64, device=x.device)
    mean32 = torch.empty((groups, (int(d) + 3) // 4 * 4), dtype=torch.float32, device=x.device) if want32 else None
    _lib.call("xv_backend_group_means", _s(), _p(x), n, ldx, int(d), _p(off_d), _p(rows_d), groups, C.c_int64(rows.size), _p(mean64), _p(mean32),
              mean32.shape[1] if want32 else 0)
    return mean64, mean32


def backend_center(x, d=None, mean=None, out=None):
    """Rows of x [rows, >= d] minus mean [d] (None: a copy) on a zero-padded pitch (xv_backend_center); out as in score_prepare."""
    rows, ldx = _pitched(x, "backend_center: x")
    d = x.shape[1] if d is None else int(d)
    if out is None:
        out = torch.empty((rows, (d + 3) // 4 * 4), dtype=torch.float32, device=x.device)
    _, ldy = _pitched(out, "backend_center: out")
    if out.shape[1] != ldy:
        raise ValueError("backend_center: out must be the whole [rows, pitch] buffer (its padding columns are written)")
    if mean is not None and (mean.dtype != torch.float32 or mean.numel() != d or not mean.is_contiguous()):
        raise ValueError("backend_center: mean must be %d contiguous float32 values" % d)
    _lib.call("xv_backend_center", _s(), _p(x), rows, d, ldx, _p(mean), _p(out), ldy)
    return out


def backend_scatter_workspace_bytes(n, d):
    return int(_lib.load().xv_backend_scatter_workspace_bytes(int(n), int(d)))


def backend_scatter(x, d=None, mean=None, ws_bytes=None):
    """[d, d] float64 = sum over the rows of x [n, >= d] of v v^T, v = x[r][:d] - mean (xv_backend_scatter).  ws_bytes: size of the
    workspace handed to the call (default: what xv_backend_scatter_workspace_bytes asks for; fewer is refused by the library)."""
    n, ldx = _pitched(x, "backend_scatter: x")
    d = x.shape[1] if d is None else int(d)
    if mean is not None and (mean.dtype != torch.float32 or mean.numel() != d or not mean.is_contiguous()):
        raise ValueError("backend_scatter: mean must be %d contiguous float32 values" % d)
    if ws_bytes is None:
        ws_bytes = backend_scatter_workspace_bytes(n, d)
    ws = torch.empty(max(int(ws_bytes) // 4, 1), dtype=torch.float32, device=x.device)
    c64 = torch.empty((max(d, 1), max(d, 1)), dtype=torch.float64, device=x.device)
    _lib.call("xv_backend_scatter", _s(), _p(x), n, d, ldx, _p(mean), _p(c64), _p(ws), C.c_size_t(int(ws_bytes)))
    return c64


def backend_plda_normalize(u, d, psi, n_utts=None, out=None):
    """u[r][:d] * sqrt(d / sum_c u_c^2 / (psi_c + 1 / n_utts[r])) (xv_backend_plda_normalize).  psi: device float32 [d]; n_utts: HOST
    integer array [rows] (None: 1 everywhere), checked positive here.  out: the [rows, pitch] tensor to write, u itself for in place;
    default a new tensor on the pitch d rounded up to 4.  Padding columns come back zero."""
    import numpy as np
    rows, ldu = _pitched(u, "backend_plda_normalize: u")
    d = int(d)
    if psi.dtype != torch.float32 or psi.numel() != d or not psi.is_contiguous():
        raise ValueError("backend_plda_normalize: psi must be %d contiguous float32 values" % d)
    if out is None:
        out = torch.empty((rows, (max(d, 1) + 3) // 4 * 4), dtype=torch.float32, device=u.device)
    _, ldo = _pitched(out, "backend_plda_normalize: out")
    if out.shape[1] != ldo:
        raise ValueError("backend_plda_normalize: out must be the whole [rows, pitch] buffer (its padding columns are written)")
    n_d = None
    if n_utts is not None:
        n_utts = _host_int(n_utts, "backend_plda_normalize: n_utts", 1, 1 << 31)
        if n_utts.size != rows:
            raise ValueError("backend_plda_normalize: n_utts must hold one count per row (%d, got %d)" % (rows, n_utts.size))
        n_d = torch.from_numpy(np.ascontiguousarray(n_utts, dtype=np.int32)).to(u.device)
    _lib.call("xv_backend_plda_normalize", _s(), _p(u), rows, d, ldu, _p(psi), _p(n_d), _p(out), ldo)
    return out


def backend_plda_trials(e, t, d, ei, ti, nidx, coef, g, k0):
    """PLDA log-likelihood ratios of trials (xv_backend_plda_trials): enrol row ei[j] of e against test row ti[j] of t, both transformed
    and normalised.  coef: device float32 [n_distinct, 2, ldc]; g: [>= d]; k0: [n_distinct]; nidx: HOST integer array [enrol rows] into the
    table.  ei, ti, nidx are checked here, before the upload: the kernel does not check indices."""
    import numpy as np
    ne, lde = _pitched(e, "backend_plda_trials: e")
    nt, ldt = _pitched(t, "backend_plda_trials: t")
    d = int(d)
    if coef.dim() != 3 or coef.shape[1] != 2 or coef.dtype != torch.float32 or not coef.is_contiguous() or coef.shape[2] < d:
        raise ValueError("backend_plda_trials: coef must be a contiguous float32 [n_distinct, 2, >= d] tensor")
    nq, ldc = coef.shape[0], coef.shape[2]
    if g.dtype != torch.float32 or g.numel() < d or not g.is_contiguous() or k0.dtype != torch.float32 or k0.numel() != nq or not k0.is_contiguous():
        raise ValueError("backend_plda_trials: g must hold >= d and k0 n_distinct contiguous float32 values")
    ei = _host_int(ei, "backend_plda_trials: ei", 0, ne)
    ti = _host_int(ti, "backend_plda_trials: ti", 0, nt)
    nidx = _host_int(nidx, "backend_plda_trials: nidx", 0, nq)
    if ei.shape != ti.shape or nidx.size != ne:
        raise ValueError("backend_plda_trials: ei and ti must be of one length, nidx one entry per enrol row")
    dev = e.device
    ei_d, ti_d, nidx_d = (torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev) for a in (ei, ti, nidx))
    out = torch.empty(ei.size, dtype=torch.float32, device=dev)
    _lib.call("xv_backend_plda_trials", _s(), _p(e), lde, ne, _p(t), ldt, nt, d, _p(ei_d), _p(ti_d), C.c_int64(ei.size), _p(nidx_d), _p(coef), ldc,
              nq, _p(g), _p(k0), _p(out))
    return out


def backend_affine(x, wt, bias):
    """x [rows, c_pad] (zero padding up to a pitch that is a multiple of 4) times wt [o, c_pad]^T plus bias [o]: the project's fp32 NT GEMM
    (xv_affine_forward, k = 1).  The caller pads wt / bias with zero rows so that o is a multiple of 4: the result is then a GEMM operand."""
    rows, ld = _pitched(x, "backend_affine: x")
    if x.shape[1] != ld or wt.shape[1] != ld or not wt.is_contiguous():
        raise ValueError("backend_affine: x must be the whole [rows, pitch] buffer and wt [o, pitch] contiguous")
    return affine_forward(x.view(rows, 1, ld), 1, wt, bias, wt.shape[0])


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
    ldn = (n + 3) // 4 * 4
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
