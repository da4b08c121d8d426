"""Op-level wrappers of the pipeline stages that take PCM (include/xvector_hip.h): MFCC, filterbank and energy VAD, augmentation and
resampling.  ops.py re-exports every public name here: callers write ops.mfcc.  Their kernels check none of the offsets, lengths and
tables they are handed, so much of this is validation - the checks these ops share are _host's - in front of one upload."""
import ctypes as C

import numpy as np
import torch

try:
    from ._host import _lib, _p, _s, config_tables, host_ints, holds_tables, pcm_samples, place_outputs, spans_inside, table_floats, upload
except ImportError:
    from _host import _lib, _p, _s, config_tables, host_ints, holds_tables, pcm_samples, place_outputs, spans_inside, table_floats, upload

mfcc_config = _lib.XvMfccConfig      # xv_mfcc_config with the VoxCeleb conf/mfcc.conf defaults (dither 0); keyword arguments name the fields to change
fbank_config = _lib.XvFbankConfig    # xv_fbank_config with compute-fbank-feats' own defaults (dither 0)


def _num_frames(kind, cfg, samples):
    name = "xv_%s_num_frames" % kind
    n = int(getattr(_lib.load(), name)(C.byref(cfg), C.c_int64(int(samples))))
    if n < 0:
        _lib.check(2, name)
    return n


def _waveform_batch(kind, cfg, tables, pcm, offsets, samples, t_out):
    """The argument checks xv_mfcc and xv_fbank share - their kernels check neither the offsets nor the tables' size - and the upload:
    -> (offsets int64 [b], samples int32 [b] on the device, b, t_out)."""
    n_pcm = pcm_samples(pcm, "%s: pcm" % kind)
    pair = "%s: offsets and samples must be two non-empty 1-D integer arrays of one length" % kind
    offsets = host_ints(offsets, min_size=1, msg=pair)
    samples = host_ints(samples, n=offsets.size, msg=pair)
    spans_inside(offsets, samples, n_pcm, "%s: an utterance lies outside the %d samples of pcm" % (kind, n_pcm))
    if samples.max() >= 2 ** 31:
        raise ValueError("%s: an utterance holds 2^31 samples or more" % kind)
    if not holds_tables(tables, table_floats(kind, cfg)) or tables.device != pcm.device:
        raise ValueError("%s: tables must be %s_tables(cfg) as a contiguous float32 device tensor" % (kind, kind))
    if t_out is None:
        t_out = max(max(_num_frames(kind, cfg, n) for n in samples), 1)
    return upload(offsets, np.int64, pcm.device), upload(samples, np.int32, pcm.device), offsets.size, int(t_out)


def mfcc_num_frames(cfg, samples):
    return _num_frames("mfcc", cfg, samples)


def mfcc_tables(cfg):
    """The constant tables of xv_mfcc for cfg as a host float32 array (xv_mfcc_tables: host arithmetic, no GPU call)."""
    return config_tables("mfcc", cfg)


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
    return config_tables("fbank", cfg)


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
    n_src, n_rir_pool, n_noise_pool = pcm_samples(src, "augment: src"), pcm_samples(rir, "augment: rir"), pcm_samples(noise, "augment: noise")
    src_off, src_len = _aug_ints(src_off, "src_off"), _aug_ints(src_len, "src_len")
    b = src_off.size
    if b == 0 or src_len.size != b:
        raise ValueError("augment: src_off and src_len must be two non-empty arrays of one length")
    spans_inside(src_off, src_len, n_src, "augment: a source is empty or lies outside the %d samples of src" % n_src, min_length=1)
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
        spans_inside(rir_off, rir_len, n_rir_pool, "augment: an impulse response is empty or lies outside the %d samples of rir" % n_rir_pool, min_length=1)
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
        spans_inside(noise_off, noise_len, n_noise_pool, "augment: a noise is empty or lies outside the %d samples of noise" % n_noise_pool, min_length=1)
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
    out_pcm, out_offsets, out_f32 = place_outputs("augment", src_len if cfg.shift_output else m_len, out_offsets, out_pcm, out_f32, src.device)
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
    return config_tables("resample", cfg)


def resample(cfg, tables, pcm, offsets, samples, out_offsets=None, out_pcm=None, out_f32=False):
    """Sample-rate conversion of a batch of waveforms (xv_resample).  tables: resample_tables(cfg) on the device; pcm: int16 device tensor,
    the utterances back to back; offsets / samples: HOST integer arrays [b] - utterance i is pcm[offsets[i] : offsets[i] + samples[i]] (the
    kernel checks nothing, so they are checked here, before the upload).  out_offsets (default: back to back) / out_pcm (default: a new
    tensor that just holds them, one sample at the least): where the outputs go; out_f32: True for a new float32 tensor of out_pcm's size,
    or such a tensor.  -> (out_pcm int16, out_offsets int64 host array, out_samples int32 [b], clipped int32 [b], out_f32 | None)."""
    n_pcm = pcm_samples(pcm, "resample: pcm")
    pair = "resample: offsets and samples must be two non-empty 1-D integer arrays of one length"
    offsets = host_ints(offsets, min_size=1, msg=pair, dtype=np.int64)
    samples = host_ints(samples, n=offsets.size, msg=pair, dtype=np.int64)
    b = offsets.size
    if b > 65535:
        raise ValueError("resample: at most 65535 utterances a call (got %d)" % b)
    spans_inside(offsets, samples, n_pcm, "resample: an utterance lies outside the %d samples of pcm" % n_pcm)
    if samples.max() >= 2 ** 31:
        raise ValueError("resample: an utterance holds 2^31 samples or more")
    floats = table_floats("resample", cfg)
    if not holds_tables(tables, floats):
        raise ValueError("resample: tables must be resample_tables(cfg) as a contiguous float32 device tensor of %d values" % floats)
    plan = resample_plan(cfg)
    n_out = (samples * plan["out_unit"] + plan["in_unit"] - 1) // plan["in_unit"]
    if n_out.max() >= 2 ** 31:
        raise ValueError("resample: an utterance would hold 2^31 samples or more")
    out_pcm, out_offsets, out_f32 = place_outputs("resample", n_out, out_offsets, out_pcm, out_f32, pcm.device, min_samples=1)
    off_d, n_d, oo_d = upload(offsets, np.int64, pcm.device), upload(samples, np.int32, pcm.device), upload(out_offsets, np.int64, pcm.device)
    out_samples = torch.empty(b, dtype=torch.int32, device=pcm.device)
    clipped = torch.empty(b, dtype=torch.int32, device=pcm.device)
    _lib.call("xv_resample", _s(), C.byref(cfg), _p(tables), _p(pcm), _p(off_d), _p(n_d), b, _p(oo_d), _p(out_pcm), _p(out_f32), _p(out_samples),
              _p(clipped))
    return out_pcm, out_offsets, out_samples, clipped, out_f32
