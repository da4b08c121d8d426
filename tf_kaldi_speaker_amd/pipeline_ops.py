"""Op-level wrappers of the pipeline stages around the network (include/xvector_hip.h): the extraction front end, MFCC, filterbank and energy
VAD, augmentation, cosine / AS-norm scoring and the LDA / PLDA back end with its cohort statistics.  ops.py re-exports every public name here: callers write ops.mfcc.
Their kernels check none of the index arrays they are handed, so much of this is validation (_host.host_ints) in front of one upload."""
import ctypes as C

import numpy as np
import torch

try:
    from ._host import _lib, _p, _s, exclusive_offsets, f32_values, host_ints, pitch4, pitched, upload
except ImportError:
    from _host import _lib, _p, _s, exclusive_offsets, f32_values, host_ints, pitch4, pitched, upload


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


CM_MAX_D = 128      # the columns the 'CM ' kernels take (CMD_MAX_D / CME_MAX_D)


def cm_decode_ragged(packed, offsets, rows, t, d):
    """'CM ' matrices as they sit in an archive behind the "CM " token, decoded on the device (xv_cm_decode_ragged; no Engine needed).
    packed: uint8 device tensor; offsets / rows: HOST integer arrays [b] - image i starts at byte offsets[i] and holds rows[i] <= t frames of d
    columns; they are checked here, before the upload.  -> float32 [b, t, d], the rows behind rows[i] zero."""
    if packed.dtype != torch.uint8 or packed.dim() != 1 or not packed.is_contiguous():
        raise ValueError("cm_decode_ragged: packed must be a contiguous 1-D uint8 tensor")
    t, d = int(t), int(d)
    if not 1 <= d <= CM_MAX_D:
        raise ValueError("cm_decode_ragged: d must lie in 1 .. %d (got %d)" % (CM_MAX_D, d))
    pair = "cm_decode_ragged: offsets and rows must be two non-empty 1-D integer arrays of one length"
    offsets = host_ints(offsets, min_size=1, msg=pair, dtype=np.int64)
    rows = host_ints(rows, "cm_decode_ragged: rows", n=offsets.size, lo=0, hi=t + 1, msg=pair, dtype=np.int64)
    if offsets.min() < 0 or (offsets + cm_image_bytes(rows, d)).max() > packed.numel():
        raise IndexError("cm_decode_ragged: an image lies outside the %d bytes of packed" % packed.numel())
    out = torch.empty((offsets.size, t, d), dtype=torch.float32, device=packed.device)
    off_d, rows_d = upload(offsets, np.int64, packed.device), upload(rows, np.int32, packed.device)
    _lib.call("xv_cm_decode_ragged", _s(), _p(packed), _p(off_d), _p(rows_d), offsets.size, t, d, _p(out))
    return out


def cm_image_bytes(rows, d):      # bytes of a 'CM ' matrix behind its token: global header, d column headers, d x rows codes
    return 16 + 8 * int(d) + int(d) * np.asarray(rows, np.int64)


def cm_encode_plan(shape, rows, header="quartiles"):
    """The checks and the offset arithmetic of cm_encode, on the host: shape = (b, t, d) of x -> (rows int32 [b], offsets int64 [b] of the
    images packed back to back, total bytes, the header's code).  Refuses by name: an unknown header, d > 128, rows[i] outside 1 .. t."""
    if header not in _lib.XV_CM_HEADERS:
        raise ValueError("cm_encode: header must be 'quartiles' or 'uniform' (got %r)" % (header,))
    b, t, d = (int(n) for n in shape)
    if not 1 <= d <= CM_MAX_D:
        raise ValueError("cm_encode: d must lie in 1 .. %d (got %d)" % (CM_MAX_D, d))
    rows = host_ints(rows, "cm_encode: rows", n=b, min_size=1, lo=1, hi=t + 1)
    sizes = cm_image_bytes(rows, d)
    return rows.astype(np.int32), exclusive_offsets(sizes), int(sizes.sum()), _lib.XV_CM_HEADERS[header]


def cm_encode(x, rows, header="quartiles"):
    """'CM ' compression of a padded batch on the device (xv_cm_encode: dataset.kaldi_io.write_compressed_mat byte for byte, in both header
    forms).  x: float32 [b, t, d] device tensor, piece i holding rows[i] frames; rows: a HOST integer array, checked here before the upload
    (1 <= rows[i] <= t; d <= 128; the header's name).  -> (uint8 device tensor: the images behind the "CM " token, packed back to back; their
    int64 host offsets [b]); image i has cm_image_bytes(rows[i], d) bytes."""
    if x.dim() != 3 or x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError("cm_encode: x must be a contiguous float32 [b, t, d] tensor")
    rows, offsets, total, code = cm_encode_plan(x.shape, rows, header)
    b, t, d = x.shape
    out = torch.empty(total, dtype=torch.uint8, device=x.device)
    rows_d, off_d = upload(rows, np.int32, x.device), upload(offsets, np.int64, x.device)
    _lib.call("xv_cm_encode", _s(), _p(x), _p(rows_d), b, t, d, code, _p(off_d), _p(out))
    return out, offsets


def _pcm(t, what):      # the samples of a pool of signals: a contiguous 1-D int16 device tensor, or None (no pool)
    if t is None:
        return 0
    if t.dtype != torch.int16 or t.dim() != 1 or not t.is_contiguous():
        raise ValueError("%s must be a contiguous 1-D int16 tensor" % what)
    return t.numel()


mfcc_config = _lib.XvMfccConfig      # xv_mfcc_config with the VoxCeleb conf/mfcc.conf defaults (dither 0); keyword arguments name the fields to change
fbank_config = _lib.XvFbankConfig    # xv_fbank_config with compute-fbank-feats' own defaults (dither 0)


def _num_frames(kind, cfg, samples):
    name = "xv_%s_num_frames" % kind
    n = int(getattr(_lib.load(), name)(C.byref(cfg), C.c_int64(int(samples))))
    if n < 0:
        _lib.check(2, name)
    return n


def _tables(kind, cfg):
    lib = _lib.load()
    n = int(getattr(lib, "xv_%s_table_floats" % kind)(C.byref(cfg)))
    if n == 0:
        _lib.check(2, "xv_%s_table_floats" % kind)
    flat = np.empty(n, np.float32)
    _lib.check(getattr(lib, "xv_%s_tables" % kind)(C.byref(cfg), C.c_void_p(flat.ctypes.data), C.c_size_t(n)), "xv_%s_tables" % kind)
    return flat


def _waveform_batch(kind, cfg, tables, pcm, offsets, samples, t_out):
    """The argument checks xv_mfcc and xv_fbank share - their kernels check neither the offsets nor the tables' size - and the upload:
    -> (offsets int64 [b], samples int32 [b] on the device, b, t_out)."""
    n_pcm = _pcm(pcm, "%s: pcm" % kind)
    pair = "%s: offsets and samples must be two non-empty 1-D integer arrays of one length" % kind
    offsets = host_ints(offsets, min_size=1, msg=pair)
    samples = host_ints(samples, n=offsets.size, msg=pair)
    if offsets.min() < 0 or samples.min() < 0 or (offsets.astype(np.int64) + samples.astype(np.int64)).max() > n_pcm:
        raise IndexError("%s: an utterance lies outside the %d samples of pcm" % (kind, n_pcm))
    if samples.max() >= 2 ** 31:
        raise ValueError("%s: an utterance holds 2^31 samples or more" % kind)
    floats = int(getattr(_lib.load(), "xv_%s_table_floats" % kind)(C.byref(cfg)))
    if floats == 0:
        _lib.check(2, "xv_%s_table_floats" % kind)
    if tables.dtype != torch.float32 or not tables.is_contiguous() or tables.numel() != floats or tables.device != pcm.device:
        raise ValueError("%s: tables must be %s_tables(cfg) as a contiguous float32 device tensor" % (kind, kind))
    if t_out is None:
        t_out = max(max(_num_frames(kind, cfg, n) for n in samples), 1)
    return upload(offsets, np.int64, pcm.device), upload(samples, np.int32, pcm.device), offsets.size, int(t_out)


def mfcc_num_frames(cfg, samples):
    return _num_frames("mfcc", cfg, samples)


def mfcc_tables(cfg):
    """The constant tables of xv_mfcc for cfg as a host float32 array (xv_mfcc_tables: host arithmetic, no GPU call)."""
    return _tables("mfcc", cfg)


def mfcc(cfg, tables, pcm, offsets, samples, t_out=None):
    """MFCCs of a batch of waveforms (xv_mfcc).  tables: mfcc_tables(cfg) on the device; pcm: int16 device tensor, the utterances back to back;
    offsets / samples: HOST integer arrays [b] - utterance i is pcm[offsets[i] : offsets[i] + samples[i]] (the kernel does not check them, so
    they are checked here, before the upload).  t_out: rows of the output (default: the longest frame count).
    -> (out [b, t_out, num_ceps] float32, rows_out int32 [b] = min(frames, t_out); rows behind are zero)."""
    off_d, n_d, b, t_out = _waveform_batch("mfcc", cfg, tables, pcm, offsets, samples, t_out)
    out = torch.empty((b, t_out, int(cfg.num_ceps)), dtype=torch.float32, device=pcm.device)
    rows_out = torch.empty(b, dtype=torch.int32, device=pcm.device)
    _lib.call("xv_mfcc", _s(), C.byref(cfg), _p(tables), _p(pcm), _p(off_d), _p(n_d), b, t_out, _p(out), _p(rows_out))
    return out, rows_out


def fbank_num_frames(cfg, samples):
    return _num_frames("fbank", cfg, samples)


def fbank_tables(cfg):
    """The constant tables of xv_fbank for cfg as a host float32 array (xv_fbank_tables: host arithmetic, no GPU call)."""
    return _tables("fbank", cfg)


def fbank(cfg, tables, pcm, offsets, samples, t_out=None, with_energy=True):
    """(Log-)mel filterbank energies of a batch of waveforms (xv_fbank); the arguments are mfcc's, with fbank_tables(cfg) as tables.
    -> (out [b, t_out, num_mel_bins + use_energy] float32, rows_out int32 [b], energy [b, t_out, 1] float32 or None without with_energy:
    the log-energy of every frame, whatever cfg.use_energy says - energy_vad(energy, rows_out) gives the decisions of an MFCC pass)."""
    off_d, n_d, b, t_out = _waveform_batch("fbank", cfg, tables, pcm, offsets, samples, t_out)
    out = torch.empty((b, t_out, int(cfg.num_mel_bins) + int(cfg.use_energy != 0)), dtype=torch.float32, device=pcm.device)
    rows_out = torch.empty(b, dtype=torch.int32, device=pcm.device)
    energy = torch.empty((b, t_out, 1), dtype=torch.float32, device=pcm.device) if with_energy else None
    _lib.call("xv_fbank", _s(), C.byref(cfg), _p(tables), _p(pcm), _p(off_d), _p(n_d), b, t_out, _p(out), _p(rows_out), _p(energy))
    return out, rows_out, energy


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


augment_config = _lib.XvAugmentConfig      # xv_augment_config with wav-reverberate's recipe settings (16 kHz, shift_output, normalize_output, no volume)


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
    h = np.asarray(h).reshape(-1)
    if h.size == 0:
        raise ValueError("augment_early: an impulse response needs at least one tap")
    p, fs = int(np.argmax(h)), np.float32(sample_frequency)
    return max(p - int(np.float32(0.001) * fs), 0), min(p + int(np.float32(0.05) * fs), h.size), p


_aug_ints = lambda a, what, n=None: host_ints(a, "augment: " + what, n=n, dtype=np.int64)


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
    n_src, n_rir_pool, n_noise_pool = _pcm(src, "augment: src"), _pcm(rir, "augment: rir"), _pcm(noise, "augment: noise")
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
    out_offsets = _aug_ints(exclusive_offsets(n_out) if out_offsets is None else out_offsets, "out_offsets", b)
    if out_pcm is None:
        out_pcm = torch.empty(int((out_offsets + n_out).max()), dtype=torch.int16, device=src.device)
    total = _pcm(out_pcm, "augment: out_pcm")
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
    tables = np.concatenate([utt_words.reshape(-1), noise_words.reshape(-1), np.stack([tile_utt, tile_first], axis=1).reshape(-1)])
    tables_d = upload(tables, np.int64, src.device)
    ws_bytes = augment_workspace_bytes(b, n_entries, n_tiles)
    ws = torch.empty((ws_bytes + 7) // 8, dtype=torch.float64, device=src.device)
    out_samples = torch.empty(b, dtype=torch.int32, device=src.device)
    clipped = torch.empty(b, dtype=torch.int32, device=src.device)
    _lib.call("xv_augment", _s(), C.byref(cfg), b, n_entries, C.c_int64(n_tiles), _p(src), _p(rir), _p(noise), _p(tables_d), C.c_size_t(tables.size),
              int(any_rir), _p(ws), C.c_size_t(ws_bytes), _p(out_pcm), _p(out_f32), _p(out_samples), _p(clipped))
    return out_pcm, out_offsets, out_samples, clipped, out_f32


def resample_config(fin, fout, num_zeros=0, cutoff=0.0):
    """xv_resample_config of the conversion fin -> fout Hz (whole numbers); zeros: the defaults (6 zeros, 0.99 * 0.5 * min(fin, fout))."""
    if int(fin) != fin or int(fout) != fout:
        raise ValueError("resample: the rates must be whole numbers of Hz (got %r -> %r)" % (fin, fout))
    return _lib.XvResampleConfig(fin=int(fin), fout=int(fout), num_zeros=int(num_zeros), cutoff=float(cutoff))


def resample_plan(cfg):
    """xv_debug_resample_plan: {in_unit, out_unit, taps_max, tile, span, lds_bytes} of cfg (host arithmetic)."""
    out = (C.c_int * 6)()
    _lib.check(_lib.load().xv_debug_resample_plan(C.byref(cfg), out), "xv_debug_resample_plan")
    return dict(in_unit=out[0], out_unit=out[1], taps_max=out[2], tile=out[3], span=out[4], lds_bytes=out[5])


def resample_num_samples(cfg, samples):
    n = int(_lib.load().xv_resample_num_samples(C.byref(cfg), C.c_int64(int(samples))))
    if n < 0:
        _lib.check(2, "xv_resample_num_samples")
    return n


def resample_tables(cfg):
    """The constant table of xv_resample for cfg as a host float32 array (xv_resample_tables: host arithmetic, no GPU call)."""
    lib = _lib.load()
    n = int(lib.xv_resample_table_floats(C.byref(cfg)))
    if n == 0:
        _lib.check(2, "xv_resample_table_floats")
    flat = np.empty(n, np.float32)
    _lib.check(lib.xv_resample_tables(C.byref(cfg), C.c_void_p(flat.ctypes.data), C.c_size_t(n)), "xv_resample_tables")
    return flat


def resample(cfg, tables, pcm, offsets, samples, out_offsets=None, out_pcm=None, out_f32=False):
    """Sample-rate conversion of a batch of waveforms (xv_resample).  tables: resample_tables(cfg) on the device; pcm: int16 device tensor,
    the utterances back to back; offsets / samples: HOST integer arrays [b] - utterance i is pcm[offsets[i] : offsets[i] + samples[i]] (the
    kernel checks nothing, so they are checked here, before the upload).  out_offsets (default: back to back) / out_pcm (default: a new
    tensor that just holds them): where the outputs go; out_f32: True for a new float32 tensor of out_pcm's size, or such a tensor.
    -> (out_pcm int16, out_offsets int64 host array, out_samples int32 [b], clipped int32 [b], out_f32 | None)."""
    n_pcm = _pcm(pcm, "resample: pcm")
    pair = "resample: offsets and samples must be two non-empty 1-D integer arrays of one length"
    offsets = host_ints(offsets, min_size=1, msg=pair, dtype=np.int64)
    samples = host_ints(samples, n=offsets.size, msg=pair, dtype=np.int64)
    b = offsets.size
    if b > 65535:
        raise ValueError("resample: at most 65535 utterances a call (got %d)" % b)
    if offsets.min() < 0 or samples.min() < 0 or (offsets + samples).max() > n_pcm:
        raise IndexError("resample: an utterance lies outside the %d samples of pcm" % n_pcm)
    if samples.max() >= 2 ** 31:
        raise ValueError("resample: an utterance holds 2^31 samples or more")
    floats = int(_lib.load().xv_resample_table_floats(C.byref(cfg)))
    if floats == 0:
        _lib.check(2, "xv_resample_table_floats")
    if tables.dtype != torch.float32 or not tables.is_contiguous() or tables.numel() != floats:
        raise ValueError("resample: tables must be resample_tables(cfg) as a contiguous float32 device tensor of %d values" % floats)
    plan = resample_plan(cfg)
    n_out = (samples * plan["out_unit"] + plan["in_unit"] - 1) // plan["in_unit"]
    if n_out.max() >= 2 ** 31:
        raise ValueError("resample: an utterance would hold 2^31 samples or more")
    out_offsets = host_ints(exclusive_offsets(n_out) if out_offsets is None else out_offsets, "resample: out_offsets", n=b, dtype=np.int64)
    if out_pcm is None:
        out_pcm = torch.empty(max(int((out_offsets + n_out).max()), 1), dtype=torch.int16, device=pcm.device)
    total = _pcm(out_pcm, "resample: out_pcm")
    order = np.argsort(out_offsets, kind="stable")
    if out_offsets.min() < 0 or (out_offsets + n_out).max() > total or (out_offsets[order][1:] < (out_offsets + n_out)[order][:-1]).any():
        raise IndexError("resample: the outputs overlap or lie outside the %d samples of out_pcm" % total)
    if out_f32 is True:
        out_f32 = torch.empty(total, dtype=torch.float32, device=pcm.device)
    elif out_f32 is False:
        out_f32 = None
    elif out_f32.dtype != torch.float32 or out_f32.dim() != 1 or not out_f32.is_contiguous() or out_f32.numel() < total:
        raise ValueError("resample: out_f32 must be a contiguous 1-D float32 tensor of out_pcm's size")
    off_d, n_d, oo_d = upload(offsets, np.int64, pcm.device), upload(samples, np.int32, pcm.device), upload(out_offsets, np.int64, pcm.device)
    out_samples = torch.empty(b, dtype=torch.int32, device=pcm.device)
    clipped = torch.empty(b, dtype=torch.int32, device=pcm.device)
    _lib.call("xv_resample", _s(), C.byref(cfg), _p(tables), _p(pcm), _p(off_d), _p(n_d), b, _p(oo_d), _p(out_pcm), _p(out_f32), _p(out_samples),
              _p(clipped))
    return out_pcm, out_offsets, out_samples, clipped, out_f32


def _centered(name, entry, x, d, mean, out):      # score_prepare and backend_center: one row-wise kernel each, on the same arguments
    rows, ldx = pitched(x, "%s: x" % name)
    d = x.shape[1] if d is None else int(d)
    if out is None:
        out = torch.empty((rows, pitch4(d)), dtype=torch.float32, device=x.device)
    _, ldy = pitched(out, "%s: out" % name, whole=True)
    if mean is not None:
        f32_values(mean, d, "%s: mean" % name)
    _lib.call(entry, _s(), _p(x), rows, d, ldx, _p(mean), _p(out), ldy)
    return out


def score_prepare(x, d=None, mean=None, out=None):
    """Rows of x [rows, >= d] minus mean [d] (None: nothing subtracted), scaled to unit length (xv_score_prepare).  d: the columns that
    hold the vector (default: all of x).  out: the [rows, ldy] tensor to write (may be x itself, in place); default a new tensor whose
    pitch is d rounded up to 4 - columns d .. ldy come back zero, so the result is a GEMM operand for score_cohort_stats."""
    return _centered("score_prepare", "xv_score_prepare", x, d, mean, out)


def score_trials(e, t, d, ei, ti, e_stats=None, t_stats=None):
    """out[j] = e[ei[j]][:d] . t[ti[j]][:d], AS-normalised with the rows' cohort statistics when both are given (xv_score_trials).
    ei, ti: HOST integer arrays (NumPy / sequences): the kernel does not check indices, so they are checked here, before the upload."""
    ne, lde = pitched(e, "score_trials: e")
    nt, ldt = pitched(t, "score_trials: t")
    pair = "score_trials: ei and ti must be two non-empty 1-D integer arrays of one length"
    ei = host_ints(ei, min_size=1, msg=pair)
    ti = host_ints(ti, n=ei.size, msg=pair)
    if ei.min() < 0 or ei.max() >= ne:
        raise IndexError("score_trials: ei holds an index outside 0 .. %d" % (ne - 1))
    if ti.min() < 0 or ti.max() >= nt:
        raise IndexError("score_trials: ti holds an index outside 0 .. %d" % (nt - 1))
    for st, n, name in ((e_stats, ne, "e_stats"), (t_stats, nt, "t_stats")):
        if st is not None and (st.dtype != torch.float32 or tuple(st.shape) != (n, 2) or not st.is_contiguous()):
            raise ValueError("score_trials: %s must be a contiguous float32 [%d, 2] tensor" % (name, n))
    ei_d, ti_d = upload(ei, np.int32, e.device), upload(ti, np.int32, e.device)
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
    rows, ldx = pitched(x, "score_cohort_stats: x")
    n_cohort, ldc = pitched(cohort, "score_cohort_stats: cohort")
    if ws_bytes is None:
        ws_bytes = score_cohort_workspace_bytes(rows, n_cohort, d)
    ws = torch.empty(max(int(ws_bytes) // 4, 1), dtype=torch.float32, device=x.device)
    stats = torch.empty((rows, 2), dtype=torch.float32, device=x.device)
    _lib.call("xv_score_cohort_stats", _s(), _p(x), ldx, rows, _p(cohort), ldc, n_cohort, int(d), int(top_k), _p(stats), _p(ws),
              C.c_size_t(int(ws_bytes)))
    return stats


def backend_group_means(x, d, offsets, rows, want32=True):
    """Averages of groups of rows of x [n, >= d] (xv_backend_group_means): group g = rows[offsets[g]:offsets[g + 1]], added in list order in
    double.  offsets, rows: HOST integer arrays (the kernel does not check them, so they are checked here: an empty group and a row outside
    x are refused).  -> (mean64 [groups, d] float64, mean32 [groups, d rounded up to 4] float32 with zero padding, or None)."""
    n, ldx = pitched(x, "backend_group_means: x")
    csr = "backend_group_means: offsets must be a 1-D integer array [groups + 1] that starts at 0"
    offsets = host_ints(offsets, min_size=2, msg=csr)
    if offsets[0] != 0:
        raise ValueError(csr)
    counts = np.diff(offsets.astype(np.int64))
    if counts.min() <= 0:
        raise ValueError("backend_group_means: group %d is empty" % int(np.argmax(counts <= 0)))
    rows = host_ints(rows, "backend_group_means: rows", min_size=1, lo=0, hi=n)
    if rows.size != int(offsets[-1]):
        raise ValueError("backend_group_means: offsets end at %d, rows holds %d indices" % (int(offsets[-1]), rows.size))
    groups = offsets.size - 1
    off_d, rows_d = upload(offsets, np.int64, x.device), upload(rows, np.int32, x.device)
    mean64 = torch.empty((groups, int(d)), dtype=torch.float64, device=x.device)
    mean32 = torch.empty((groups, pitch4(int(d))), dtype=torch.float32, device=x.device) if want32 else None
    _lib.call("xv_backend_group_means", _s(), _p(x), n, ldx, int(d), _p(off_d), _p(rows_d), groups, C.c_int64(rows.size), _p(mean64), _p(mean32),
              mean32.shape[1] if want32 else 0)
    return mean64, mean32


def backend_center(x, d=None, mean=None, out=None):
    """Rows of x [rows, >= d] minus mean [d] (None: a copy) on a zero-padded pitch (xv_backend_center); out as in score_prepare."""
    return _centered("backend_center", "xv_backend_center", x, d, mean, out)


def backend_scatter_workspace_bytes(n, d):
    return int(_lib.load().xv_backend_scatter_workspace_bytes(int(n), int(d)))


def backend_scatter(x, d=None, mean=None, ws_bytes=None):
    """[d, d] float64 = sum over the rows of x [n, >= d] of v v^T, v = x[r][:d] - mean (xv_backend_scatter).  ws_bytes: size of the
    workspace handed to the call (default: what xv_backend_scatter_workspace_bytes asks for; fewer is refused by the library)."""
    n, ldx = pitched(x, "backend_scatter: x")
    d = x.shape[1] if d is None else int(d)
    if mean is not None:
        f32_values(mean, d, "backend_scatter: mean")
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
    rows, ldu = pitched(u, "backend_plda_normalize: u")
    d = int(d)
    f32_values(psi, d, "backend_plda_normalize: psi")
    if out is None:
        out = torch.empty((rows, pitch4(max(d, 1))), dtype=torch.float32, device=u.device)
    _, ldo = pitched(out, "backend_plda_normalize: out", whole=True)
    n_d = None
    if n_utts is not None:
        n_utts = host_ints(n_utts, "backend_plda_normalize: n_utts", min_size=1, lo=1, hi=1 << 31)
        if n_utts.size != rows:
            raise ValueError("backend_plda_normalize: n_utts must hold one count per row (%d, got %d)" % (rows, n_utts.size))
        n_d = upload(n_utts, np.int32, u.device)
    _lib.call("xv_backend_plda_normalize", _s(), _p(u), rows, d, ldu, _p(psi), _p(n_d), _p(out), ldo)
    return out


def backend_plda_trials(e, t, d, ei, ti, nidx, coef, g, k0):
    """PLDA log-likelihood ratios of trials (xv_backend_plda_trials): enrol row ei[j] of e against test row ti[j] of t, both transformed
    and normalised.  coef: device float32 [n_distinct, 2, ldc]; g: [>= d]; k0: [n_distinct]; nidx: HOST integer array [enrol rows] into the
    table.  ei, ti, nidx are checked here, before the upload: the kernel does not check indices."""
    ne, lde = pitched(e, "backend_plda_trials: e")
    nt, ldt = pitched(t, "backend_plda_trials: t")
    d = int(d)
    nq, ldc = _plda_tables("backend_plda_trials", coef, g, k0, d)
    ei = host_ints(ei, "backend_plda_trials: ei", min_size=1, lo=0, hi=ne)
    ti = host_ints(ti, "backend_plda_trials: ti", min_size=1, lo=0, hi=nt)
    nidx = host_ints(nidx, "backend_plda_trials: nidx", min_size=1, lo=0, hi=nq)
    if ei.shape != ti.shape or nidx.size != ne:
        raise ValueError("backend_plda_trials: ei and ti must be of one length, nidx one entry per enrol row")
    ei_d, ti_d, nidx_d = (upload(a, np.int32, e.device) for a in (ei, ti, nidx))
    out = torch.empty(ei.size, dtype=torch.float32, device=e.device)
    _lib.call("xv_backend_plda_trials", _s(), _p(e), lde, ne, _p(t), ldt, nt, d, _p(ei_d), _p(ti_d), C.c_int64(ei.size), _p(nidx_d), _p(coef), ldc,
              nq, _p(g), _p(k0), _p(out))
    return out


def _plda_tables(name, coef, g, k0, d):      # the checks plda_trials and plda_cohort_stats share: -> (n_distinct, pitch of coef)
    if coef.dim() != 3 or coef.shape[1] != 2 or coef.dtype != torch.float32 or not coef.is_contiguous() or coef.shape[2] < d:
        raise ValueError("%s: coef must be a contiguous float32 [n_distinct, 2, >= d] tensor" % name)
    nq = coef.shape[0]
    if g.dtype != torch.float32 or g.numel() < d or not g.is_contiguous() or k0.dtype != torch.float32 or k0.numel() != nq or not k0.is_contiguous():
        raise ValueError("%s: g must hold >= d and k0 n_distinct contiguous float32 values" % name)
    return nq, coef.shape[2]


def backend_plda_cohort_workspace_bytes(rows, n_cohort, d, n_distinct):
    return int(_lib.load().xv_backend_plda_cohort_workspace_bytes(int(rows), int(n_cohort), int(d), int(n_distinct)))


def backend_plda_cohort_stats(x, cohort, d, nidx, coef, g, k0, top_k, ws_bytes=None):
    """[rows, 2] = (mean, biased deviation) of each row's min(top_k, n_cohort) largest PLDA log-likelihood ratios against the cohort rows
    (xv_backend_plda_cohort_stats).  x: PLDA-normalised rows in the model role (backend_plda_normalize with their utterance counts), cohort:
    rows normalised with one utterance; both on a zero-padded pitch that is a multiple of 4.  coef, g, k0: plda_coefficients' tables on the
    device; nidx: HOST integer array [rows] into them (None: entry 0 for every row), checked here before the upload.  ws_bytes: size of
    the workspace (default: the whole call in one round); fewer bytes run the rows in tiles."""
    rows, ldx = pitched(x, "backend_plda_cohort_stats: x")
    n_cohort, ldc = pitched(cohort, "backend_plda_cohort_stats: cohort")
    d = int(d)
    nq, ldk = _plda_tables("backend_plda_cohort_stats", coef, g, k0, d)
    nidx_d = None
    if nidx is not None:
        nidx = host_ints(nidx, "backend_plda_cohort_stats: nidx", min_size=1, lo=0, hi=nq)
        if nidx.size != rows:
            raise ValueError("backend_plda_cohort_stats: nidx must hold one entry per row (%d, got %d)" % (rows, nidx.size))
        nidx_d = upload(nidx, np.int32, x.device)
    if ws_bytes is None:
        ws_bytes = backend_plda_cohort_workspace_bytes(rows, n_cohort, d, nq)
    ws = torch.empty(max(int(ws_bytes) // 4, 1), dtype=torch.float32, device=x.device)
    stats = torch.empty((rows, 2), dtype=torch.float32, device=x.device)
    _lib.call("xv_backend_plda_cohort_stats", _s(), _p(x), ldx, rows, _p(nidx_d), _p(cohort), ldc, n_cohort, d, _p(coef), ldk, nq, _p(g), _p(k0),
              int(top_k), _p(stats), _p(ws), C.c_size_t(int(ws_bytes)))
    return stats


def score_normalize(scores, ei, ti, e_stats, t_stats, out=None):
    """AS-norm of scores that are on the device already (xv_score_normalize): out[j] = 0.5 * ((s - mu_e) / sigma_e + (s - mu_t) / sigma_t),
    s = scores[j], the statistics those of rows ei[j] of e_stats [ne, 2] and ti[j] of t_stats [nt, 2] - score_trials' expression, bit for
    bit.  ei, ti: HOST integer arrays, checked here before the upload.  out: the tensor to write (scores itself: in place); default new."""
    if scores.dim() != 1 or scores.dtype != torch.float32 or not scores.is_contiguous() or scores.numel() == 0:
        raise ValueError("score_normalize: scores must be a non-empty contiguous 1-D float32 tensor")
    for st, name in ((e_stats, "e_stats"), (t_stats, "t_stats")):
        if st is None or st.dtype != torch.float32 or st.dim() != 2 or st.shape[1] != 2 or not st.is_contiguous() or st.shape[0] == 0:
            raise ValueError("score_normalize: %s must be a contiguous float32 [n, 2] tensor" % name)
    m = scores.numel()
    ei = host_ints(ei, "score_normalize: ei", n=m, lo=0, hi=e_stats.shape[0])
    ti = host_ints(ti, "score_normalize: ti", n=m, lo=0, hi=t_stats.shape[0])
    if out is None:
        out = torch.empty(m, dtype=torch.float32, device=scores.device)
    elif out.dtype != torch.float32 or out.dim() != 1 or out.numel() != m or not out.is_contiguous():
        raise ValueError("score_normalize: out must be a contiguous 1-D float32 tensor of the scores' length")
    ei_d, ti_d = upload(ei, np.int32, scores.device), upload(ti, np.int32, scores.device)
    _lib.call("xv_score_normalize", _s(), _p(scores), _p(ei_d), _p(ti_d), C.c_int64(m), _p(e_stats), _p(t_stats), _p(out))
    return out
