"""Waveforms on the host, for features.py, augment.py and resample.py and their drivers: RIFF PCM-16 files and the scp files that list
them, lists of waveforms as the one packed int16 tensor the ops read, and what is said once about sample rates - grouping by rate,
compute-mfcc-feats' allow rule and its refusal, the kept Resamplers."""
import collections
import io
import os
import wave

import numpy as np

try:
    from .._host import DEFAULT_WORKSPACE_BYTES, exclusive_offsets, upload
except (ImportError, ValueError):
    from _host import DEFAULT_WORKSPACE_BYTES, exclusive_offsets, upload

# What read_wav_rate asks of its options: the rate and channel to read and which conversions pass.  features.MfccOptions and FbankOptions
# carry the same four fields; the defaults are theirs (16 kHz, a mono file, no resampling).
WavFormat = collections.namedtuple("WavFormat", "sample_frequency channel allow_downsample allow_upsample")
WavFormat.__new__.__defaults__ = (16000.0, -1, 0, 0)


def rate_allowed(options, rate):
    """compute-mfcc-feats' rule for a file at another rate than options.sample_frequency: a higher one needs allow_downsample, a lower one
    allow_upsample."""
    return bool(options.allow_downsample if rate > options.sample_frequency else options.allow_upsample)


def rate_refusal(options, rate, who="", resampling=True):
    """The text that refuses such a file; who: what names it, in front; resampling False: the reader that never converts (read_wav)."""
    return "%ssample rate %d Hz, but --sample-frequency=%g (there is no resampling%s)" % (
        who and who + ": ", rate, options.sample_frequency,
        "" if not resampling else " without --allow-downsample=true" if rate > options.sample_frequency else " without --allow-upsample=true")


def read_wav(rxfilename, options=None, key=""):
    """The samples of a RIFF PCM-16 file as an int16 array: a path or a `cmd |` entry of a wav.scp (dataset.kaldi_io.open_or_fd), read with the
    stdlib wave module.  options (a WavFormat, or MfccOptions): the sample rate must be options.sample_frequency, and options.channel picks
    the channel (-1: the file must be mono).  Anything else is refused, naming `key`."""
    return read_wav_rate(rxfilename, options, key, any_rate=False)[0]


def read_wav_rate(rxfilename, options=None, key="", any_rate=None):
    """(samples, sample rate in Hz) of a file as read_wav reads it.  any_rate None: a file at another rate than options.sample_frequency
    passes if options allows the conversion (rate_allowed); True: every rate passes (the caller resamples); False: read_wav's refusal.
    The samples come back at the FILE's rate."""
    try:
        from ..dataset import kaldi_io
    except (ImportError, ValueError):
        from dataset import kaldi_io
    options = options or WavFormat()
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
        rate = w.getframerate()
        if rate != int(options.sample_frequency) or int(options.sample_frequency) != options.sample_frequency:
            allowed = rate_allowed(options, rate) if any_rate is None else any_rate
            if not allowed or rate < 1 or int(options.sample_frequency) != options.sample_frequency:
                raise ValueError(rate_refusal(options, rate, who, any_rate is not False))
        channels = w.getnchannels()
        x = np.frombuffer(w.readframes(w.getnframes()), dtype="<i2").reshape(-1, channels)
    if options.channel < 0:
        if channels != 1:
            raise ValueError("%s: %d channels; choose one with --channel" % (who, channels))
        return np.ascontiguousarray(x[:, 0]), rate
    if options.channel >= channels:
        raise ValueError("%s: --channel=%d, but the file has %d channel(s)" % (who, options.channel, channels))
    return np.ascontiguousarray(x[:, options.channel]), rate


def write_wav(path, samples, sample_frequency):
    """A mono RIFF PCM-16 file (stdlib wave)."""
    with wave.open(path, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(int(sample_frequency))
        w.writeframes(np.ascontiguousarray(samples, dtype="<i2").tobytes())


def scp_entries(path, numbered=True):
    """(key, rxfilename) of every `key rxfilename` line of a Kaldi scp file, as the lines are reached; a malformed one is refused where
    it stands - numbered: with its line number."""
    with open(path, "r") as f:
        for number, line in enumerate(f, 1):
            line = line.strip()
            if not line:
                continue
            parts = line.split(None, 1)
            if len(parts) != 2:
                raise ValueError("%s: `key rxfilename` is expected, got `%s`" % ("%s:%d" % (path, number) if numbered else path, line))
            yield parts[0], parts[1]


def read_scp(path):
    """[(key, rxfilename)] of a Kaldi scp file."""
    return list(scp_entries(path))


def read_wav_scp(path, options):
    """(key, samples, sample rate) of every `key rxfilename` line of a wav.scp, read by read_wav_rate under options' rate rules - the
    reader of make_mfcc.py, make_fbank.py and extract.py's wav mode.  ValueError: a malformed line, or what read_wav_rate refuses."""
    for key, rx in scp_entries(path, numbered=False):
        wav, rate = read_wav_rate(rx, options, key)
        yield key, wav, rate


class WavDir(object):
    """out_dir/wav/<key>.wav, the files a driver writes: write() -> the `key path` line of out_dir/wav.scp."""

    def __init__(self, out_dir):
        self.wav_dir, self.scp_path = os.path.join(out_dir, "wav"), os.path.join(out_dir, "wav.scp")
        os.makedirs(self.wav_dir, exist_ok=True)

    def write(self, key, samples, sample_frequency):
        path = os.path.join(self.wav_dir, key + ".wav")
        write_wav(path, samples, sample_frequency)
        return "%s %s\n" % (key, path)


def pack(waves, device):
    """Waveforms (int16 arrays) back to back, as the ops read them: -> (pcm: an int16 tensor on `device`, None when there is no sample;
    offsets int64 [b]; lengths int64 [b]) - utterance i is pcm[offsets[i] : offsets[i] + lengths[i]]."""
    waves = [np.ascontiguousarray(w, dtype=np.int16).reshape(-1) for w in waves]
    lengths = np.asarray([w.size for w in waves], np.int64)
    pcm = upload(np.concatenate(waves), np.int16, device) if lengths.sum() else None
    return pcm, exclusive_offsets(lengths) if waves else np.zeros(0, np.int64), lengths


def unpack(pcm, offsets, lengths):
    """pack's inverse on the host: [int16 array per utterance], copies."""
    host = pcm.cpu().numpy()
    return [host[o:o + k].copy() for o, k in zip(offsets, lengths)]


def by_rate(rates):
    """{rate: [i, ...]} of a list of sample rates (Hz; None: the entry is in no group), the rates in the order they first appear."""
    groups = {}
    for i, rate in enumerate(rates):
        if rate is not None:
            groups.setdefault(int(rate), []).append(i)
    return groups


class Resamplers(dict):
    """{(fin, fout): resample.Resampler} of a device, each built when it is first asked for and kept: its table goes to the device once."""

    def __init__(self, device, workspace_bytes=DEFAULT_WORKSPACE_BYTES):
        dict.__init__(self)
        self.device, self.workspace_bytes = device, workspace_bytes

    def __missing__(self, rates):
        try:
            from .resample import Resampler
        except (ImportError, ValueError):
            from misc.resample import Resampler
        self[rates] = Resampler(rates[0], rates[1], self.device, self.workspace_bytes)
        return self[rates]

    @classmethod
    def of(cls, owner):
        """The cache of an object with a device and workspace_bytes (a FeatureExtractor, an Augmenter), made when it is first asked for."""
        if "_resamplers" not in owner.__dict__:
            owner._resamplers = cls(owner.device, owner.workspace_bytes)
        return owner._resamplers
