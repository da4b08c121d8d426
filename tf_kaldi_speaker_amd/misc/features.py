"""MFCC features and energy VAD decisions from waveforms on the GPU: the host side of xv_mfcc / xv_energy_vad (include/xvector_hip.h), what
steps/make_mfcc.sh --mfcc-config conf/mfcc.conf and sid/compute_vad_decision.sh do in the reference recipe (egs/voxceleb/v1/run.sh:59-63).

    mfcc = MfccOptions.from_conf("conf/mfcc.conf")           # Kaldi --name=value lines; what is not supported is refused by name
    vad = VadOptions.from_conf("conf/vad.conf")
    fx = FeatureExtractor(mfcc, vad, "cuda:0")
    for feats, decisions in fx.extract([read_wav(rx, mfcc, key) for key, rx in entries]): ...

This is the --dither=0 program: Kaldi's default dither of 1.0 adds noise from its own generator and is not reproducible across Kaldi runs
either.  Defaults are the VoxCeleb conf's (30 bins, 30 coefficients, 20 - 7600 Hz, snip-edges false), NOT compute-mfcc-feats' own: a conf
file should state what it relies on."""
import io
import wave

import numpy as np

try:
    from .._host import DEFAULT_WORKSPACE_BYTES, _lib, device_ops, exclusive_offsets, greedy_batches
except (ImportError, ValueError):
    from _host import DEFAULT_WORKSPACE_BYTES, _lib, device_ops, exclusive_offsets, greedy_batches

_TRUE, _FALSE = ("true", "t", "1"), ("false", "f", "0")


def _bool(name, text):
    if text.lower() in _TRUE:
        return 1
    if text.lower() in _FALSE:
        return 0
    raise ValueError("--%s=%s: true or false is expected" % (name, text))


def _conf_lines(path):
    """(name, value) of every `--name=value` line of a Kaldi conf file; `#` starts a comment."""
    out = []
    with open(path, "r") as f:
        for number, line in enumerate(f, 1):
            line = line.split("#", 1)[0].strip()
            if not line:
                continue
            if not line.startswith("--") or "=" not in line:
                raise ValueError("%s:%d: `--name=value` is expected, got `%s`" % (path, number, line))
            name, value = line[2:].split("=", 1)
            out.append((name.strip(), value.strip()))
    return out


class _Options(object):
    """Options by Kaldi name.  SUPPORTED: name -> (attribute, parser).  FIXED: options of the Kaldi program that this one does not
    implement, name -> (the one value that changes nothing, parser): that value is accepted, any other is refused by name."""
    SUPPORTED, FIXED, PROGRAM = {}, {}, ""

    def __init__(self, **kw):
        for attr, _ in self.SUPPORTED.values():
            setattr(self, attr, self.DEFAULTS[attr])
        for k, v in kw.items():
            if k not in self.DEFAULTS:
                raise TypeError("%s: no option `%s`" % (type(self).__name__, k))
            setattr(self, k, v)

    def set(self, name, text):
        if name in self.SUPPORTED:
            attr, parse = self.SUPPORTED[name]
            setattr(self, attr, parse(name, text))
        elif name in self.FIXED:
            only, parse = self.FIXED[name]
            if parse(name, text) != only:
                raise ValueError("--%s=%s is not supported (only --%s=%s: %s)" % (name, text, name, str(only).lower(), self.WHY.get(name, "not implemented")))
        else:
            raise ValueError("--%s is not an option of %s that this program knows" % (name, self.PROGRAM))

    @classmethod
    def from_conf(cls, path):
        self = cls()
        for name, value in _conf_lines(path):
            self.set(name, value)
        return self


def _f(name, text):
    try:
        return float(text)
    except ValueError:
        raise ValueError("--%s=%s: a number is expected" % (name, text))


def _i(name, text):
    try:
        return int(text)
    except ValueError:
        raise ValueError("--%s=%s: a whole number is expected" % (name, text))


def _s(name, text):
    return text


class MfccOptions(_Options):
    """The options of compute-mfcc-feats this program takes; fields are those of xv_mfcc_config plus `channel` (-1: the file must be mono)."""
    PROGRAM = "compute-mfcc-feats"
    DEFAULTS = dict(_lib.XvMfccConfig.DEFAULTS, channel=-1)
    SUPPORTED = {"sample-frequency": ("sample_frequency", _f), "frame-length": ("frame_length_ms", _f), "frame-shift": ("frame_shift_ms", _f),
                 "num-mel-bins": ("num_mel_bins", _i), "num-ceps": ("num_ceps", _i), "low-freq": ("low_freq", _f), "high-freq": ("high_freq", _f),
                 "snip-edges": ("snip_edges", _bool), "preemphasis-coefficient": ("preemphasis", _f), "remove-dc-offset": ("remove_dc_offset", _bool),
                 "cepstral-lifter": ("cepstral_lifter", _f), "use-energy": ("use_energy", _bool), "raw-energy": ("raw_energy", _bool),
                 "energy-floor": ("energy_floor", _f), "channel": ("channel", _i)}
    FIXED = {"dither": (0.0, _f), "window-type": ("povey", _s), "htk-compat": (0, _bool), "round-to-power-of-two": (1, _bool),
             "vtln-warp": (1.0, _f), "vtln-map": ("", _s), "utt2spk": ("", _s), "vtln-low": (100.0, _f), "vtln-high": (-500.0, _f),
             "subtract-mean": (0, _bool), "blackman-coeff": (0.42, _f), "allow-downsample": (0, _bool), "allow-upsample": (0, _bool),
             "debug-mel": (0, _bool), "min-duration": (0.0, _f), "output-format": ("kaldi", _s), "max-feature-vectors": (-1, _i)}
    WHY = {"dither": "dither is random and not reproducible; on digital silence use --energy-floor", "window-type": "the window is Povey's",
           "allow-downsample": "no resampling", "allow-upsample": "no resampling", "vtln-warp": "no VTLN", "vtln-map": "no VTLN", "utt2spk": "no VTLN",
           "vtln-low": "no VTLN", "vtln-high": "no VTLN", "subtract-mean": "extract.py --cmn-window normalises"}

    def config(self):
        """The xv_mfcc_config of these options."""
        return _lib.XvMfccConfig(**{k: getattr(self, k) for k in self.DEFAULTS if k != "channel"})


class VadOptions(_Options):
    """The options of compute-vad-decision; the defaults are the VoxCeleb conf/vad.conf (5.5, 0.5, 2, 0.12), not the program's own."""
    PROGRAM = "compute-vad-decision"
    DEFAULTS = dict(threshold=5.5, mean_scale=0.5, frames_context=2, proportion=0.12)
    SUPPORTED = {"vad-energy-threshold": ("threshold", _f), "vad-energy-mean-scale": ("mean_scale", _f), "vad-frames-context": ("frames_context", _i),
                 "vad-proportion-threshold": ("proportion", _f)}
    FIXED, WHY = {}, {}


def read_wav(rxfilename, options=None, key=""):
    """The samples of a RIFF PCM-16 file as an int16 array: a path or a `cmd |` entry of a wav.scp (dataset.kaldi_io.open_or_fd), read with the
    stdlib wave module.  options (MfccOptions): the sample rate must be options.sample_frequency, and options.channel picks the channel
    (-1: the file must be mono).  Anything else is refused, naming `key`."""
    try:
        from ..dataset import kaldi_io
    except (ImportError, ValueError):
        from dataset import kaldi_io
    options = options or MfccOptions()
    who = "Key %s (%s)" % (key, rxfilename) if key else rxfilename
    fd = kaldi_io.open_or_fd(rxfilename, "rb")
    try:
        data = fd.read()
    finally:
        fd.close()
    try:
        w = wave.open(io.BytesIO(data), "rb")
    except (wave.Error, EOFError) as e:
        raise ValueError("%s: not a RIFF PCM file (%s)" % (who, e))
    with w:
        if w.getsampwidth() != 2:
            raise ValueError("%s: %d-bit samples; only PCM-16 is read" % (who, 8 * w.getsampwidth()))
        if w.getframerate() != int(options.sample_frequency) or int(options.sample_frequency) != options.sample_frequency:
            raise ValueError("%s: sample rate %d Hz, but --sample-frequency=%g (there is no resampling)" % (who, w.getframerate(), options.sample_frequency))
        channels = w.getnchannels()
        x = np.frombuffer(w.readframes(w.getnframes()), dtype="<i2").reshape(-1, channels)
    if options.channel < 0:
        if channels != 1:
            raise ValueError("%s: %d channels; choose one with --channel" % (who, channels))
        return np.ascontiguousarray(x[:, 0])
    if options.channel >= channels:
        raise ValueError("%s: --channel=%d, but the file has %d channel(s)" % (who, options.channel, channels))
    return np.ascontiguousarray(x[:, options.channel])


class FeatureExtractor(object):
    """MFCCs and VAD decisions of waveforms.  The constant tables are built once (xv_mfcc_tables, host arithmetic) and kept on the device;
    extract() cuts its list into batches such that the padded outputs and the samples of one call stay within workspace_bytes."""

    def __init__(self, mfcc=None, vad=None, device="cuda:0", workspace_bytes=DEFAULT_WORKSPACE_BYTES):
        self.torch, self.ops, self.device = device_ops(device)
        self.mfcc, self.vad = mfcc or MfccOptions(), vad or VadOptions()
        self.cfg = self.mfcc.config()
        self.tables = self.torch.from_numpy(self.ops.mfcc_tables(self.cfg)).to(self.device)
        self.workspace_bytes = int(workspace_bytes)

    def num_frames(self, samples):
        return self.ops.mfcc_num_frames(self.cfg, samples)

    def _cost(self, b, t_max, total):
        return b * max(t_max, 1) * (4 * self.mfcc.num_ceps + 1) + 2 * total

    def _batches(self, frames, lengths):
        grow = lambda i, b=0, t_max=0, total=0: (b + 1, max(t_max, frames[i]), total + lengths[i])
        too_big = lambda i, cost: ("FeatureExtractor: a workspace of %d bytes does not hold utterance %d (%d samples, %d frames: %d bytes)"
                                   % (self.workspace_bytes, i, lengths[i], frames[i], cost))
        return greedy_batches(len(frames), grow, self._cost, self.workspace_bytes, max_items=65535, too_big=too_big)

    def extract(self, waves):
        """waves: int16 arrays -> [(features float32 [T, num_ceps], decisions float32 [T] of 1.0 / 0.0)] in order; T may be 0."""
        waves = [np.ascontiguousarray(w, dtype=np.int16).reshape(-1) for w in waves]
        lengths = [len(w) for w in waves]
        frames = [self.num_frames(n) for n in lengths]
        out = [None] * len(waves)
        for batch in self._batches(frames, lengths):
            n = [lengths[i] for i in batch]
            if sum(n) == 0:
                for i in batch:
                    out[i] = (np.zeros((0, self.mfcc.num_ceps), np.float32), np.zeros(0, np.float32))
                continue
            pcm = self.torch.from_numpy(np.concatenate([waves[i] for i in batch])).to(self.device)
            for i, r in zip(batch, self.extract_packed(pcm, exclusive_offsets(n), n)):      # one call: the batch fits
                out[i] = r
        return out

    def extract_packed(self, pcm, offsets, lengths):
        """The same for utterances that are on the device already: pcm an int16 device tensor, utterance i its samples offsets[i] ..
        offsets[i] + lengths[i] (host arrays) - what misc.augment.Augmenter.run returns.  Nothing is copied; the calls are cut as by
        extract()."""
        ops, v = self.ops, self.vad
        offsets, lengths = np.asarray(offsets, np.int64), [int(n) for n in lengths]
        frames = [self.num_frames(n) for n in lengths]
        out = [None] * len(lengths)
        for batch in self._batches(frames, lengths):
            if sum(lengths[i] for i in batch) == 0:
                for i in batch:
                    out[i] = (np.zeros((0, self.mfcc.num_ceps), np.float32), np.zeros(0, np.float32))
                continue
            t_out = max(max(frames[i] for i in batch), 1)
            x, rows = ops.mfcc(self.cfg, self.tables, pcm, offsets[batch], np.asarray([lengths[i] for i in batch], np.int64), t_out)
            masks = ops.energy_vad(x, rows, v.threshold, v.mean_scale, v.frames_context, v.proportion)
            x_h, m_h, r_h = x.cpu().numpy(), masks.cpu().numpy(), rows.cpu().numpy()
            for j, i in enumerate(batch):
                assert r_h[j] == frames[i], (i, r_h[j], frames[i])
                out[i] = (x_h[j, :frames[i]].copy(), m_h[j, :frames[i]].astype(np.float32))
        return out
