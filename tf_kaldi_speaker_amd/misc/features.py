"""MFCC or filterbank features and energy VAD decisions from waveforms on the GPU: the host side of xv_mfcc / xv_fbank / xv_energy_vad
(include/xvector_hip.h), what steps/make_mfcc.sh --mfcc-config conf/mfcc.conf (steps/make_fbank.sh --fbank-config conf/fbank.conf) and
sid/compute_vad_decision.sh do in the reference recipe (egs/voxceleb/v1/run.sh:59-63).

    mfcc = MfccOptions.from_conf("conf/mfcc.conf")           # Kaldi --name=value lines; what is not supported is refused by name
    vad = VadOptions.from_conf("conf/vad.conf")
    fx = FeatureExtractor(mfcc, vad, "cuda:0")
    for feats, decisions in fx.extract([read_wav(rx, mfcc, key) for key, rx in entries]): ...

This is the --dither=0 program: Kaldi's default dither of 1.0 adds noise from its own generator and is not reproducible across Kaldi runs
either.  MfccOptions' defaults are the VoxCeleb conf's (30 bins, 30 coefficients, 20 - 7600 Hz, snip-edges false), NOT compute-mfcc-feats'
own: a conf file should state what it relies on.  FbankOptions' defaults are compute-fbank-feats' own.  The readers of wav files and of a
wav.scp, and what is common to everything that handles waveforms and their rates, are misc/waves.py's; the conf parser is misc/conf.py's."""
import numpy as np

try:
    from .._host import DEFAULT_WORKSPACE_BYTES, _lib, device_ops, exclusive_offsets, greedy_batches
    from . import waves as W
    from .conf import _Options, _bool, _f, _i, _s
    from .waves import read_wav, read_wav_rate, read_wav_scp      # noqa: F401 (drivers and tests reach the readers of misc/waves.py here)
except (ImportError, ValueError):
    from _host import DEFAULT_WORKSPACE_BYTES, _lib, device_ops, exclusive_offsets, greedy_batches
    from misc import waves as W
    from misc.conf import _Options, _bool, _f, _i, _s
    from misc.waves import read_wav, read_wav_rate, read_wav_scp      # noqa: F401


class MfccOptions(_Options):
    """The options of compute-mfcc-feats this program takes; fields are those of xv_mfcc_config plus `channel` (-1: the file must be mono) and
    allow_downsample / allow_upsample (0: a file at another rate is refused; 1: it is resampled on the device, misc/resample.py)."""
    PROGRAM = "compute-mfcc-feats"
    HOST_ONLY = ("channel", "allow_downsample", "allow_upsample")      # what is not a field of xv_mfcc_config
    DEFAULTS = dict(_lib.XvMfccConfig.DEFAULTS, channel=-1, allow_downsample=0, allow_upsample=0)
    SUPPORTED = {"sample-frequency": ("sample_frequency", _f), "frame-length": ("frame_length_ms", _f), "frame-shift": ("frame_shift_ms", _f),
                 "num-mel-bins": ("num_mel_bins", _i), "num-ceps": ("num_ceps", _i), "low-freq": ("low_freq", _f), "high-freq": ("high_freq", _f),
                 "snip-edges": ("snip_edges", _bool), "preemphasis-coefficient": ("preemphasis", _f), "remove-dc-offset": ("remove_dc_offset", _bool),
                 "cepstral-lifter": ("cepstral_lifter", _f), "use-energy": ("use_energy", _bool), "raw-energy": ("raw_energy", _bool),
                 "energy-floor": ("energy_floor", _f), "channel": ("channel", _i), "allow-downsample": ("allow_downsample", _bool),
                 "allow-upsample": ("allow_upsample", _bool)}
    FIXED = {"dither": (0.0, _f), "window-type": ("povey", _s), "htk-compat": (0, _bool), "round-to-power-of-two": (1, _bool),
             "vtln-warp": (1.0, _f), "vtln-map": ("", _s), "utt2spk": ("", _s), "vtln-low": (100.0, _f), "vtln-high": (-500.0, _f),
             "subtract-mean": (0, _bool), "blackman-coeff": (0.42, _f),
             "debug-mel": (0, _bool), "min-duration": (0.0, _f), "output-format": ("kaldi", _s), "max-feature-vectors": (-1, _i)}
    WHY = {"dither": "dither is random and not reproducible; on digital silence use --energy-floor", "window-type": "the window is Povey's",
           "vtln-warp": "no VTLN", "vtln-map": "no VTLN", "utt2spk": "no VTLN",
           "vtln-low": "no VTLN", "vtln-high": "no VTLN", "subtract-mean": "extract.py --cmn-window normalises"}

    KIND = "mfcc"      # the ops that take config(): ops.mfcc, ops.mfcc_tables, ops.mfcc_num_frames

    def config(self):
        """The xv_mfcc_config of these options."""
        return _lib.XvMfccConfig(**{k: getattr(self, k) for k in self.DEFAULTS if k not in self.HOST_ONLY})

    def feature_dim(self):
        return int(self.num_ceps)


class FbankOptions(_Options):
    """The options of compute-fbank-feats this program takes; fields are those of xv_fbank_config plus MfccOptions' host-side ones (channel,
    allow_downsample, allow_upsample).  The defaults are compute-fbank-feats' own (23 bins, 20 Hz .. the Nyquist frequency, snip-edges
    true, no energy column): Kaldi's fbank confs rely on them.  What is refused, and why, is what MfccOptions refuses."""
    PROGRAM = "compute-fbank-feats"
    KIND = "fbank"
    HOST_ONLY = MfccOptions.HOST_ONLY
    DEFAULTS = dict(_lib.XvFbankConfig.DEFAULTS, channel=-1, allow_downsample=0, allow_upsample=0)
    SUPPORTED = dict({name: spec for name, spec in MfccOptions.SUPPORTED.items() if name not in ("num-ceps", "cepstral-lifter")},
                     **{"use-log-fbank": ("use_log_fbank", _bool), "use-power": ("use_power", _bool)})
    FIXED, WHY = MfccOptions.FIXED, MfccOptions.WHY

    def config(self):
        """The xv_fbank_config of these options."""
        return _lib.XvFbankConfig(**{k: getattr(self, k) for k in self.DEFAULTS if k not in self.HOST_ONLY})

    def feature_dim(self):
        return int(self.num_mel_bins) + (1 if self.use_energy else 0)


class VadOptions(_Options):
    """The options of compute-vad-decision; the defaults are the VoxCeleb conf/vad.conf (5.5, 0.5, 2, 0.12), not the program's own."""
    PROGRAM = "compute-vad-decision"
    DEFAULTS = dict(threshold=5.5, mean_scale=0.5, frames_context=2, proportion=0.12)
    SUPPORTED = {"vad-energy-threshold": ("threshold", _f), "vad-energy-mean-scale": ("mean_scale", _f), "vad-frames-context": ("frames_context", _i),
                 "vad-proportion-threshold": ("proportion", _f)}
    FIXED, WHY = {}, {}


class FeatureExtractor(object):
    """Features (MFCCs or filterbank energies) and VAD decisions of waveforms.  mfcc: a MfccOptions or a FbankOptions - the kernel follows
    the option set.  The constant tables are built once (xv_mfcc_tables / xv_fbank_tables, host arithmetic) and kept on the device;
    extract() cuts its list into batches such that the padded outputs and the samples of one call stay within workspace_bytes.  The VAD
    reads the log-energy: column 0 of the MFCCs (the conf must keep --use-energy=true, as Kaldi's does), xv_fbank's energy_out for
    filterbanks - whatever their --use-energy says, so an fbank system needs no second feature pass for its decisions.  with_vad False:
    no decisions are computed, None stands in their place."""

    def __init__(self, mfcc=None, vad=None, device="cuda:0", workspace_bytes=DEFAULT_WORKSPACE_BYTES, with_vad=True):
        self.torch, self.ops, self.device = device_ops(device)
        self.mfcc, self.vad = mfcc or MfccOptions(), vad or VadOptions()      # self.mfcc: the feature options of either kind
        self.cfg = self.mfcc.config()
        self.tables = self.torch.from_numpy(getattr(self.ops, self.kind + "_tables")(self.cfg)).to(self.device)
        self.workspace_bytes, self.with_vad = int(workspace_bytes), bool(with_vad)

    kind = property(lambda self: self.mfcc.KIND)                 # "mfcc" or "fbank": the ops that take cfg
    dim = property(lambda self: self.mfcc.feature_dim())        # floats per frame

    def num_frames(self, samples):
        return getattr(self.ops, self.kind + "_num_frames")(self.cfg, samples)

    def on_device(self, pcm, offsets, lengths, t_out):
        """One call on utterances that are on the device (extract_packed's arguments, not cut): -> (features [b, t_out, dim], rows int32 [b],
        masks uint8 [b, t_out] or None without with_vad), device tensors - the layout ops.frontend and the engine read."""
        ops, v, with_vad = self.ops, self.vad, self.with_vad
        if self.kind == "fbank":
            x, rows, energy = ops.fbank(self.cfg, self.tables, pcm, offsets, lengths, t_out, with_energy=with_vad)
        else:
            x, rows = ops.mfcc(self.cfg, self.tables, pcm, offsets, lengths, t_out)
            energy = x
        masks = ops.energy_vad(energy, rows, v.threshold, v.mean_scale, v.frames_context, v.proportion) if with_vad else None
        return x, rows, masks

    def _cost(self, b, t_max, total, coded=False):      # coded: the 'CM ' images as well, a byte per value; + 4: fbank's energy column
        return b * max(t_max, 1) * ((5 if coded else 4) * self.dim + 1 + (4 if self.kind == "fbank" else 0)) + 2 * total

    def _batches(self, frames, lengths, coded=False):
        grow = lambda i, b=0, t_max=0, total=0: (b + 1, max(t_max, frames[i]), total + lengths[i])
        too_big = lambda i, cost: ("FeatureExtractor: a workspace of %d bytes does not hold utterance %d (%d samples, %d frames: %d bytes)"
                                   % (self.workspace_bytes, i, lengths[i], frames[i], cost))
        cost_of = lambda b, t_max, total: self._cost(b, t_max, total, coded)
        return greedy_batches(len(frames), grow, cost_of, self.workspace_bytes, max_items=65535, too_big=too_big)

    def _nothing(self, cm_header):      # what an utterance too short for one frame gives
        return (np.zeros((0, self.dim), np.float32) if cm_header is None else b"", np.zeros(0, np.float32) if self.with_vad else None)

    def extract(self, waves, cm_header=None):
        """waves: int16 arrays -> [(features float32 [T, dim], decisions float32 [T] of 1.0 / 0.0)] in order; T may be 0.
        cm_header ("uniform" or "quartiles"): the features come back 'CM '-compressed on the device instead (ops.cm_encode: the bytes
        dataset.kaldi_io.write_compressed_mat(header=cm_header) gives for the float features) - [(the image behind the "CM " token, a bytes-like
        object, empty when T is 0; decisions)]: a byte per value crosses to the host instead of four."""
        lengths = [np.size(w) for w in waves]
        out = [None] * len(waves)
        for batch in self._batches([self.num_frames(n) for n in lengths], lengths, cm_header is not None):
            packed = W.pack([waves[i] for i in batch], self.device)      # one upload and one call: the batch fits
            for i, r in zip(batch, self.extract_packed(*packed, cm_header=cm_header)):
                out[i] = r
        return out

    def resampler(self, rate):
        """The Resampler rate -> sample_frequency of this extractor, kept: its table goes to the device once."""
        return W.Resamplers.of(self)[rate, self.mfcc.sample_frequency]

    def _rate_groups(self, waves, rates):
        """(members, pcm, offsets, lengths) per sample rate among `rates` (Hz, whole numbers), in the order the rates first appear: the
        members' waveforms packed on the device at sample_frequency - uploaded as they are, or resampled there (rounded to int16;
        compute-mfcc-feats keeps floats: unpinned).  A higher rate needs mfcc.allow_downsample, a lower one
        mfcc.allow_upsample.  pcm is None when a group at sample_frequency holds no sample."""
        for rate, members in W.by_rate(rates).items():
            group = [waves[i] for i in members]
            if rate == self.mfcc.sample_frequency:
                yield (members,) + W.pack(group, self.device)
            elif not W.rate_allowed(self.mfcc, rate):
                raise ValueError(W.rate_refusal(self.mfcc, rate))
            else:
                yield (members,) + self.resampler(rate).run(group)[:3]

    def extract_at_rates(self, waves, rates, cm_header=None):
        """extract() for waveforms at their own sample rates: those at sample_frequency go through as they are, the others are resampled
        on the device, grouped by rate, and reach xv_mfcc as int16 without leaving it (_rate_groups)."""
        out = [None] * len(waves)
        for members, pcm, offsets, lengths in self._rate_groups(waves, rates):
            for i, r in zip(members, self.extract_packed(pcm, offsets, lengths, cm_header)):
                out[i] = r
        return out

    def device_batches(self, waves, rates):
        """extract_at_rates for a consumer on the device (extract.py's wav mode): one feature call per sample rate among `rates`, the
        others resampled first, and NOTHING is read back but one int32 per utterance - how many frames its mask keeps (without with_vad
        all of them, and nothing at all is read).  Yields (members: the indices into waves, samples per member at sample_frequency,
        kaldi_io.DeviceBatch or None when no member holds a sample).  The caller bounds the list: one call holds its padded features."""
        try:
            from ..dataset.kaldi_io import DeviceBatch
        except (ImportError, ValueError):
            from dataset.kaldi_io import DeviceBatch
        for members, pcm, offsets, lengths in self._rate_groups(waves, rates):
            lengths = [int(n) for n in lengths]
            if pcm is None:
                yield members, lengths, None
                continue
            frames = [self.num_frames(n) for n in lengths]
            x, rows, masks = self.on_device(pcm, offsets, np.asarray(lengths, np.int64), max(max(frames), 1))
            kept = frames if masks is None else masks.sum(dim=1, dtype=self.torch.int32).cpu().tolist()
            yield members, lengths, DeviceBatch(x, rows, masks, frames, kept)

    def extract_packed(self, pcm, offsets, lengths, cm_header=None):
        """The same for utterances that are on the device already: pcm an int16 device tensor, utterance i its samples offsets[i] ..
        offsets[i] + lengths[i] (host arrays) - what misc.augment.Augmenter.run returns.  Nothing is copied; the calls are cut as by
        extract()."""
        ops = self.ops
        offsets, lengths = np.asarray(offsets, np.int64), [int(n) for n in lengths]
        frames = [self.num_frames(n) for n in lengths]
        out = [None] * len(lengths)
        for batch in self._batches(frames, lengths, cm_header is not None):
            if sum(lengths[i] for i in batch) == 0:
                for i in batch:
                    out[i] = self._nothing(cm_header)
                continue
            t_out = max(max(frames[i] for i in batch), 1)
            x, rows, masks = self.on_device(pcm, offsets[batch], np.asarray([lengths[i] for i in batch], np.int64), t_out)
            r_h = rows.cpu().numpy()
            decisions = (lambda j, i: None) if masks is None else (lambda j, i, m_h=masks.cpu().numpy(): m_h[j, :frames[i]].astype(np.float32))
            for j, i in enumerate(batch):
                assert r_h[j] == frames[i], (i, r_h[j], frames[i])
            if cm_header is None:
                x_h = x.cpu().numpy()
                for j, i in enumerate(batch):
                    out[i] = (x_h[j, :frames[i]].copy(), decisions(j, i))
                continue
            kept = [j for j, i in enumerate(batch) if frames[i] > 0]      # a 'CM ' matrix has at least one row
            if len(kept) < len(batch):
                x = x[self.torch.as_tensor(kept, device=x.device)] if kept else None
            images = iter(encoded_images(ops, x, [frames[batch[j]] for j in kept], cm_header) if kept else ())
            for j, i in enumerate(batch):
                out[i] = (next(images) if frames[i] > 0 else b"", decisions(j, i))
        return out


def encoded_images(ops, x, rows, cm_header):
    """ops.cm_encode on a padded batch, copied back: [the image of piece i behind its "CM " token, a view into the one host buffer]."""
    buf, offsets = ops.cm_encode(x, np.asarray(rows, np.int64), header=cm_header)
    raw = memoryview(buf.cpu().numpy())
    return [raw[int(o):int(o + n)] for o, n in zip(offsets, ops.cm_image_bytes(rows, x.shape[2]))]


def rows_of(feats, d):
    """Frames of what FeatureExtractor.extract returns for an utterance: a float matrix, or a 'CM ' image of d columns (empty: none)."""
    if isinstance(feats, np.ndarray):
        return int(feats.shape[0])
    return (len(feats) - 16 - 8 * d) // d if len(feats) else 0


def write_cm_image(fd, image, key=""):
    """`key `, the "\\0BCM " token and an image as ops.cm_encode leaves it: what dataset.kaldi_io.write_compressed_mat writes for the matrix."""
    if key != "":
        fd.write((key + " ").encode("latin1"))
    fd.write(b"\0BCM ")
    fd.write(image)


class FeaturePreparer(object):
    """The training features of the recipe from raw ones, on the device: what prepare_feats_for_egs.sh pipes through Kaldi
    (egs/voxceleb/v1/run.sh stage 4: apply-cmvn-sliding --norm-vars=false --center=true --cmn-window=300 | select-voiced-frames |
    copy-feats --compress=true) as decode -> ops.frontend -> ops.cm_encode.  prepare() cuts its list into calls whose buffers - the
    archive bytes, the decoded and the normalised batch, the selected indices, the masks and the images - stay within workspace_bytes."""

    def __init__(self, cmn_window=300, cm_header="uniform", device="cuda:0", workspace_bytes=DEFAULT_WORKSPACE_BYTES):
        self.torch, self.ops, self.device = device_ops(device)
        if cmn_window < 0:
            raise ValueError("FeaturePreparer: cmn_window must be 0 (off) or a number of frames")
        self.ops.cm_encode_plan((1, 1, 1), [1], cm_header)      # the header's name, before any work
        self.cmn_window, self.cm_header, self.workspace_bytes = int(cmn_window), cm_header, int(workspace_bytes)

    @staticmethod
    def _cost(b, t_max, v_max, d, packed):
        return packed + b * (max(t_max, 1) * (4 * d + 1) + max(v_max, 1) * (4 * d + 4 + d) + 16 + 8 * d)

    def prepare(self, items, masks):
        """items: the RAW utterances, dataset.kaldi_io.PackedMatrix ('CM ' as it sits in the archive: decoded on the device) or float32
        matrices; masks: per utterance one uint8 per frame, non-zero = voiced, with at least one voiced frame - or None: every frame is kept.
        -> [the 'CM ' image of the normalised, selected utterance, behind its token] in order; its rows = the voiced count."""
        n_in = [int(f.shape[0]) for f in items]
        masks = [None if m is None else np.ascontiguousarray(np.asarray(m) != 0).view(np.uint8) for m in masks]
        n_out = [n if m is None else int(np.count_nonzero(m)) for n, m in zip(n_in, masks)]
        for i, (f, m) in enumerate(zip(items, masks)):
            if (m is not None and m.shape != (n_in[i],)) or n_out[i] < 1 or f.shape[1] != items[0].shape[1]:
                raise ValueError("FeaturePreparer: utterance %d: %d frames of %d columns, %s decisions, %d voiced (one mask byte per frame, a "
                                 "voiced frame and one dimension for all are expected)" % (i, n_in[i], f.shape[1], "no" if m is None else m.size, n_out[i]))
        if not items:
            return []
        d = int(items[0].shape[1])
        size = lambda i: len(items[i].payload) if hasattr(items[i], "payload") else 0
        grow = lambda i, b=0, t=0, v=0, packed=0: (b + 1, max(t, n_in[i]), max(v, n_out[i]), packed + size(i))
        cost_of = lambda b, t, v, packed: self._cost(b, t, v, d, packed)
        too_big = lambda i, cost: ("FeaturePreparer: a workspace of %d bytes does not hold utterance %d (%d frames: %d bytes)"
                                   % (self.workspace_bytes, i, n_in[i], cost))
        out = [None] * len(items)
        for batch in greedy_batches(len(items), grow, cost_of, self.workspace_bytes, max_items=65535, too_big=too_big):
            for i, image in zip(batch, self._call([items[i] for i in batch], [masks[i] for i in batch], [n_out[i] for i in batch], d)):
                out[i] = image
        return out

    def _call(self, items, masks, n_out, d):
        torch, ops = self.torch, self.ops
        n_in = np.asarray([f.shape[0] for f in items], np.int64)
        t_in = int(n_in.max())
        if all(hasattr(f, "payload") for f in items):      # the archive bytes go up as they are
            sizes = [len(f.payload) for f in items]
            packed = torch.from_numpy(np.concatenate([np.frombuffer(f.payload, np.uint8) for f in items])).to(self.device)
            x = ops.cm_decode_ragged(packed, exclusive_offsets(sizes), n_in, t_in, d)
        else:
            x_h = np.zeros((len(items), t_in, d), np.float32)
            for j, f in enumerate(items):
                x_h[j, :n_in[j]] = f.decode() if hasattr(f, "payload") else f
            x = torch.from_numpy(x_h).to(self.device)
        rows_in = torch.from_numpy(n_in.astype(np.int32)).to(self.device)
        if any(m is not None for m in masks):
            masks = [np.ones(n, np.uint8) if m is None else m for n, m in zip(n_in, masks)]
            m_d = torch.from_numpy(np.concatenate(masks)).to(self.device)
            mo_d = torch.from_numpy(exclusive_offsets([len(m) for m in masks])).to(self.device)
            y, _ = ops.frontend(x, rows_in, self.cmn_window, masks=m_d, mask_offsets=mo_d, t_out=max(n_out))
        else:
            y, _ = ops.frontend(x, rows_in, self.cmn_window, t_out=max(n_out))
        return encoded_images(ops, y, n_out, self.cm_header)
