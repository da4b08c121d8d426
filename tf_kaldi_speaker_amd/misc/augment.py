"""Reverberation and additive-noise augmentation of waveforms on the GPU: the host side of xv_augment (include/xvector_hip.h), what the
`wav-reverberate` pipes in the augmented wav.scp entries of the reference recipe do (egs/voxceleb/v1/run.sh:68-130).

    options = AugmentOptions.from_conf("conf/augment.conf")      # Kaldi --name=value lines; what is not supported is refused by name
    entries = read_plan("plan", 16000.0)                         # out_key src_key [speed=F] [rir=ID] [noise=ID:snr:start_seconds[:bg]] ...
    aug = Augmenter(options, rirs, noises, 16000.0, "cuda:0")    # rirs / noises: {id: int16 array}
    pcm, offsets, lengths, clipped = aug.run(sources, entries)   # the packed int16 device tensor FeatureExtractor.extract_packed reads

A plan line names one output utterance: its source, at most one impulse response and any number of noises in the order they are added - a
foreground noise is added once at start_seconds, `:bg` marks a background noise, repeated over the whole utterance (what
augment_data_dir.py reaches through wav-reverberate --duration).  `speed=F` (at most one a line) perturbs the source first: it is resampled
F * fs -> fs (misc/resample.py; 0.9 makes it longer and lower) before the impulse response and the noises meet it.  The arithmetic is
wav-reverberate's with --normalize-output=true AS RESTATED in the header.  Every file must have the sample rate of the sources, unless
read_signals is told to pass the impulse responses and noises with their rates (--resample-signals true): the Augmenter then resamples those
that differ when it builds its pools."""
import numpy as np

from . import resample
from .features import DEFAULT_WORKSPACE_BYTES, _Options, _bool, _f, _i, _lib, device_ops, exclusive_offsets, greedy_batches

PRESETS = {"reverb": None, "noise": (15.0, 10.0, 5.0, 0.0), "music": (15.0, 10.0, 8.0, 5.0), "babble": (20.0, 17.0, 15.0, 13.0)}


class AugmentOptions(_Options):
    """The options of wav-reverberate this program takes.  The signals and their SNRs and start times come from the plan, not from options."""
    PROGRAM = "wav-reverberate"
    DEFAULTS = dict(shift_output=1, normalize_output=1, volume=0.0, impulse_response_channel=0, noise_channel=0)
    SUPPORTED = {"shift-output": ("shift_output", _bool), "normalize-output": ("normalize_output", _bool), "volume": ("volume", _f),
                 "impulse-response-channel": ("impulse_response_channel", _i), "noise-channel": ("noise_channel", _i)}
    FIXED, WHY = {}, {}
    REFUSED = {"duration": "use a background noise entry (noise=ID:snr:0:bg) in the plan",
               "multi-channel-output": "one channel is written",
               "input-wave-channel": "use --channel of the MFCC conf",
               "impulse-response": "the plan names the impulse response (rir=ID)",
               "additive-signals": "the plan names the noises (noise=ID:snr:start_seconds[:bg])",
               "snrs": "the plan carries the SNR of each noise", "start-times": "the plan carries the start of each noise",
               "noise-file": "the plan names the noises (noise=ID:snr:start_seconds[:bg])", "snr-db": "the plan carries the SNR of each noise"}

    def set(self, name, text):
        if name in self.REFUSED:
            raise ValueError("--%s is not supported: %s" % (name, self.REFUSED[name]))
        _Options.set(self, name, text)
        if self.volume < 0 or self.impulse_response_channel < 0 or self.noise_channel < 0:
            raise ValueError("--%s=%s: must not be negative" % (name, text))

    def config(self, sample_frequency):
        """The xv_augment_config of these options."""
        return _lib.XvAugmentConfig(sample_frequency=sample_frequency, shift_output=self.shift_output, normalize_output=self.normalize_output,
                                    volume=self.volume)


class PlanEntry(object):
    """One output utterance: noises = [(id, snr dB, start sample, background)]; speed: None, or the factor as the decimal text of the plan
    (`0.9`) - the source is resampled speed * fs -> fs BEFORE the impulse response and the noises, so n, the noise starts and
    --shift-output refer to the perturbed length."""
    __slots__ = ("out_key", "src_key", "rir", "noises", "speed")

    def __init__(self, out_key, src_key, rir=None, noises=(), speed=None):
        self.out_key, self.src_key, self.rir, self.noises = out_key, src_key, rir, list(noises)
        self.speed = None if speed is None else _speed_text(speed)

    def line(self, sample_frequency):
        parts = [self.out_key, self.src_key] + (["speed=%s" % self.speed] if self.speed is not None else [])
        parts += ["rir=%s" % self.rir] if self.rir is not None else []
        for nid, snr, start, bg in self.noises:
            seconds = start / float(sample_frequency)
            if start_sample(seconds, sample_frequency) != start:      # the fp32 product fell just below the whole number: aim at its middle
                seconds = (start + 0.5) / float(sample_frequency)
            assert start_sample(seconds, sample_frequency) == start
            parts.append("noise=%s:%r:%s%s" % (nid, float(snr), repr(seconds) if start else "0", ":bg" if bg else ""))
        return " ".join(parts)


def _speed_text(speed):      # a factor as the plan writes it: 0.9 -> `0.9`, "1.10" -> `1.10`
    return repr(speed) if isinstance(speed, float) else str(speed)


def start_sample(seconds, sample_frequency):
    """seconds * sample_frequency in fp32, truncated - Kaldi's `time * samp_freq`."""
    return int(np.float32(seconds) * np.float32(sample_frequency))


def read_plan(path, sample_frequency=16000.0, rir_ids=None, noise_ids=None):
    """The entries of a plan file.  Anything that is not understood - a field, a number, an id that rir_ids / noise_ids (containers, when
    given) do not hold, an output key used twice - fails with the file, the line number and the offending text."""
    entries, seen = [], set()
    with open(path, "r") as f:
        for number, line in enumerate(f, 1):
            line = line.split("#", 1)[0].strip()
            if not line:
                continue
            where = "%s:%d" % (path, number)
            parts = line.split()
            if len(parts) < 2 or "=" in parts[0] or "=" in parts[1]:
                raise ValueError("%s: `out_key src_key [rir=ID] [noise=ID:snr:start_seconds[:bg]] ...` is expected, got `%s`" % (where, line))
            if parts[0] in seen:
                raise ValueError("%s: output key %s is used twice" % (where, parts[0]))
            seen.add(parts[0])
            entry = PlanEntry(parts[0], parts[1])
            for field in parts[2:]:
                name, eq, value = field.partition("=")
                if name == "rir" and eq and value:
                    if entry.rir is not None:
                        raise ValueError("%s: a second impulse response `%s` (one per utterance)" % (where, field))
                    if rir_ids is not None and value not in rir_ids:
                        raise ValueError("%s: impulse response %s is not in the table of impulse responses" % (where, value))
                    entry.rir = value
                elif name == "noise" and eq and value:
                    bits = value.split(":")
                    if len(bits) not in (3, 4) or (len(bits) == 4 and bits[3] != "bg") or not bits[0]:
                        raise ValueError("%s: `noise=ID:snr:start_seconds[:bg]` is expected, got `%s`" % (where, field))
                    try:
                        snr, seconds = float(bits[1]), float(bits[2])
                    except ValueError:
                        raise ValueError("%s: the SNR and the start of `%s` must be numbers" % (where, field))
                    if not (np.isfinite(snr) and abs(snr) <= 200 and np.isfinite(seconds) and seconds >= 0):
                        raise ValueError("%s: `%s`: an SNR within +-200 dB and a start >= 0 s are expected" % (where, field))
                    background = len(bits) == 4
                    if background and seconds != 0:
                        raise ValueError("%s: `%s`: a background noise covers the whole utterance, its start must be 0" % (where, field))
                    if noise_ids is not None and bits[0] not in noise_ids:
                        raise ValueError("%s: noise %s is not in the table of noises" % (where, bits[0]))
                    entry.noises.append((bits[0], snr, start_sample(seconds, sample_frequency), background))
                elif name == "speed" and eq and value:
                    if entry.speed is not None:
                        raise ValueError("%s: a second speed `%s` (one per utterance)" % (where, field))
                    try:
                        resample.speed_rates(value, sample_frequency)
                    except ValueError as e:
                        raise ValueError("%s: `%s`: %s" % (where, field, e))
                    entry.speed = value
                else:
                    raise ValueError("%s: unknown field `%s` (rir=ID, noise=ID:snr:start_seconds[:bg] and speed=F are known)" % (where, field))
            entries.append(entry)
    return entries


def write_plan(entries, path, sample_frequency=16000.0):
    with open(path, "w") as f:
        for e in entries:
            f.write(e.line(sample_frequency) + "\n")


def make_plan(preset, utterances, rirs=(), noises=(), seed=0, fg_interval=1.0, sample_frequency=16000.0):
    """One of the recipe's four lists, seeded (numpy.random.RandomState(seed)).  utterances / rirs / noises: [(key or id, seconds)].
      reverb  `key-reverb`: one impulse response per utterance
      noise   `key-noise`:  foreground noises from 0 s on, each fg_interval seconds behind the end of the one before, SNRs of 15:10:5:0
      music   `key-music`:  one background noise, 15:10:8:5
      babble  `key-babble`: three to seven background noises, 20:17:15:13
    The random choices are THIS project's: they do not reproduce those of Kaldi's steps/data/reverberate_data_dir.py and
    augment_data_dir.py, which draw from Python's own generator in an order of their own."""
    if preset not in PRESETS:
        raise ValueError("make_plan: unknown preset `%s` (%s are known)" % (preset, ", ".join(sorted(PRESETS))))
    rs = np.random.RandomState(seed)
    pool = list(rirs if preset == "reverb" else noises)
    if not pool:
        raise ValueError("make_plan: the `%s` list needs a table of %s" % (preset, "impulse responses" if preset == "reverb" else "noises"))
    if fg_interval < 0:
        raise ValueError("make_plan: --fg-interval must not be negative")
    snrs = PRESETS[preset]
    entries = []
    for key, seconds in utterances:
        entry = PlanEntry("%s-%s" % (key, preset), key)
        if preset == "reverb":
            entry.rir = pool[rs.randint(len(pool))][0]
        elif preset == "noise":
            t = 0.0
            while t < seconds:
                nid, length = pool[rs.randint(len(pool))]
                entry.noises.append((nid, snrs[rs.randint(len(snrs))], start_sample(t, sample_frequency), False))
                t += max(float(length), 1.0 / sample_frequency) + fg_interval
        else:
            for _ in range(1 if preset == "music" else rs.randint(3, 8)):
                entry.noises.append((pool[rs.randint(len(pool))][0], snrs[rs.randint(len(snrs))], 0, True))
        entries.append(entry)
    return entries


def make_speed_plan(utterances, factors, sample_frequency=16000.0):
    """The speed-perturbed copies of a list: for each factor F, in order, a line `sp<F>-<key> <key> speed=<F>` per utterance.  utterances:
    keys, or (key, seconds) as make_plan takes them; factors: decimal texts or floats (0.9, 1.1).  F * sample_frequency must be a whole
    number and F lie in 0.5 .. 2."""
    entries = []
    for factor in factors:
        text = _speed_text(factor)
        try:
            resample.speed_rates(text, sample_frequency)
        except ValueError as e:
            raise ValueError("make_speed_plan: %s" % e)
        for u in utterances:
            key = u if isinstance(u, str) else u[0]
            entries.append(PlanEntry("sp%s-%s" % (text, key), key, speed=text))
    return entries


def read_scp(path):
    """[(key, rxfilename)] of a Kaldi scp file."""
    out = []
    with open(path, "r") as f:
        for number, line in enumerate(f, 1):
            if not line.strip():
                continue
            parts = line.strip().split(None, 1)
            if len(parts) != 2:
                raise ValueError("%s:%d: `key rxfilename` is expected, got `%s`" % (path, number, line.strip()))
            out.append((parts[0], parts[1]))
    return out


def read_signals(scp_path, sample_frequency, channel, what, resample_signals=False):
    """{id: int16 array} of a rir.scp / noise.scp style table: `id rxfilename` lines, RIFF PCM-16 at the sources' sample rate (without
    resample_signals there is no resampling; a mismatch is refused as by read_wav), `channel` of each file.  resample_signals: every rate
    passes and the table is {id: (int16 array, its rate in Hz)} - the Augmenter converts those that differ when it builds its pools."""
    from . import features
    opts = features.MfccOptions(sample_frequency=sample_frequency, channel=channel)
    out = {}
    for key, rx in read_scp(scp_path):
        if key in out:
            raise ValueError("%s: %s %s is listed twice" % (scp_path, what, key))
        samples, rate = features.read_wav_rate(rx, opts, key, any_rate=bool(resample_signals))
        out[key] = (samples, rate) if resample_signals else samples
        if len(samples) == 0:
            raise ValueError("%s: %s %s holds no samples" % (scp_path, what, key))
    return out


def signal_seconds(signals, sample_frequency):
    """[(id, seconds)] of a read_signals table in either form (what make_plan takes)."""
    return [(k, len(v[0]) / float(v[1])) if isinstance(v, tuple) else (k, len(v) / float(sample_frequency)) for k, v in signals.items()]


def write_wav(path, samples, sample_frequency):
    """A mono RIFF PCM-16 file (stdlib wave)."""
    import wave
    with wave.open(path, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(int(sample_frequency))
        w.writeframes(np.ascontiguousarray(samples, dtype="<i2").tobytes())


class Augmenter(object):
    """Keeps the impulse responses and the noises on the device (int16, back to back) and runs lists of plan entries in calls whose
    workspace and sources stay within workspace_bytes."""

    def __init__(self, options=None, rirs=None, noises=None, sample_frequency=16000.0, device="cuda:0", workspace_bytes=DEFAULT_WORKSPACE_BYTES):
        self.torch, self.ops, self.device = device_ops(device)
        self.options = options or AugmentOptions()
        self.sample_frequency = float(sample_frequency)
        self.cfg = self.options.config(self.sample_frequency)
        self.workspace_bytes = int(workspace_bytes)
        self.tile = self.ops.augment_plan(1)["tile"]
        self._resamplers = {}
        rirs, noises = self._at_rate(rirs or {}), self._at_rate(noises or {})
        self.rir_index, self.rir_pool, self.rir_off, self.rir_len = self._pool(rirs, "impulse response")
        self.noise_index, self.noise_pool, self.noise_off, self.noise_len = self._pool(noises, "noise")
        self.rir_early = [self.ops.augment_early(rirs[k], self.sample_frequency) for k in self.rir_index] if rirs else []

    def resampler(self, fin):
        """The Resampler fin -> sample_frequency of this Augmenter, kept: its table goes to the device once."""
        if fin not in self._resamplers:
            self._resamplers[fin] = resample.Resampler(fin, self.sample_frequency, self.device, self.workspace_bytes)
        return self._resamplers[fin]

    def _at_rate(self, signals):
        """A read_signals table in either form as {id: int16 array at sample_frequency}: the (array, rate) entries whose rate differs are
        resampled on the device, once, grouped by rate (xv_resample; rounded to int16, as the wav of a `sox -r` stage is)."""
        out = {k: (v[0] if isinstance(v, tuple) else v) for k, v in signals.items()}
        groups = {}
        for k, v in signals.items():
            if isinstance(v, tuple) and int(v[1]) != self.sample_frequency:
                groups.setdefault(int(v[1]), []).append(k)
        for rate, keys in groups.items():
            converted, _ = self.resampler(rate).resample([signals[k][0] for k in keys])
            out.update(zip(keys, converted))
        return out

    def perturbed(self, sources, entries):
        """The sources of the entries with speed=F resampled F * fs -> fs on the device, grouped by factor, and brought back as int16 (the
        intermediate a piped wav would be); the others as they are."""
        sources = list(sources)
        groups = {}
        for i, e in enumerate(entries):
            if e.speed is not None:
                groups.setdefault(resample.speed_rates(e.speed, self.sample_frequency)[0], []).append(i)
        for fin, members in groups.items():
            converted, _ = self.resampler(fin).resample([sources[i] for i in members])
            for i, w in zip(members, converted):
                sources[i] = w
        return sources

    def _pool(self, signals, what):
        keys = list(signals)
        arrays = [np.ascontiguousarray(signals[k], dtype=np.int16).reshape(-1) for k in keys]
        for k, a in zip(keys, arrays):
            if a.size == 0:
                raise ValueError("Augmenter: %s %s holds no samples" % (what, k))
        lengths = np.asarray([a.size for a in arrays], np.int64)
        offsets = exclusive_offsets(lengths) if keys else np.zeros(0, np.int64)
        pool = self.torch.from_numpy(np.concatenate(arrays)).to(self.device) if keys else None
        return {k: i for i, k in enumerate(keys)}, pool, offsets, lengths

    def lengths(self, sources, entries):
        """(M, n_out) per entry: the samples of y and of the output (step 6)."""
        return self._lengths([self.source_samples(len(s), e) for s, e in zip(sources, entries)], entries)

    def source_samples(self, n, entry):
        """The samples of a source of n samples as the entry's impulse response and noises meet it: ceil(n / speed) under speed=F."""
        if entry.speed is None:
            return n
        fin, fout = resample.speed_rates(entry.speed, self.sample_frequency)
        return 0 if n <= 0 else -(-n * fout // fin)      # ceil(n * out_unit / in_unit): the common divisor cancels

    def _lengths(self, n, entries):
        n = np.asarray(n, np.int64)
        taps = np.asarray([self.rir_len[self.rir_index[e.rir]] if e.rir is not None else 0 for e in entries], np.int64)
        m = np.where(taps > 0, n + taps - 1, n)
        return m, (n if self.options.shift_output else m)

    def _cost(self, tiles, entries, samples, utts):
        return self.ops.augment_workspace_bytes(utts, entries, tiles) + 2 * samples

    def _batches(self, n, m, entries):
        grow = lambda i, tiles=0, noises=0, samples=0, utts=0: (tiles + int((m[i] + self.tile - 1) // self.tile), noises + len(entries[i].noises),
                                                                samples + int(n[i]), utts + 1)
        too_big = lambda i, cost: ("Augmenter: a workspace of %d bytes does not hold utterance %d (%s: %d samples under %d taps: %d bytes)"
                                   % (self.workspace_bytes, i, entries[i].out_key, n[i], m[i] - n[i] + 1 if entries[i].rir is not None else 0, cost))
        return greedy_batches(len(entries), grow, self._cost, self.workspace_bytes, too_big=too_big)

    def run(self, sources, entries):
        """sources[i]: the int16 samples of entries[i].src_key -> (pcm int16 device tensor, offsets int64 [b], lengths int64 [b], clipped
        int64 [b]), host arrays but for pcm: utterance i is pcm[offsets[i] : offsets[i] + lengths[i]], the layout ops.mfcc reads."""
        torch, ops = self.torch, self.ops
        if len(sources) != len(entries) or not entries:
            raise ValueError("Augmenter: one source per plan entry is needed, and at least one entry")
        sources = [np.ascontiguousarray(s, dtype=np.int16).reshape(-1) for s in sources]
        for e, s in zip(entries, sources):
            if len(s) == 0:
                raise ValueError("Augmenter: Key %s: the source %s holds no samples" % (e.out_key, e.src_key))
            if e.rir is not None and e.rir not in self.rir_index:
                raise KeyError("Augmenter: Key %s: impulse response %s is not in the table of impulse responses" % (e.out_key, e.rir))
            for nid, _, _, _ in e.noises:
                if nid not in self.noise_index:
                    raise KeyError("Augmenter: Key %s: noise %s is not in the table of noises" % (e.out_key, nid))
        if any(e.speed is not None for e in entries):
            sources = self.perturbed(sources, entries)
        n = np.asarray([len(s) for s in sources], np.int64)
        m, n_out = self._lengths(n, entries)
        offsets = exclusive_offsets(n_out)
        pcm = torch.empty(int(n_out.sum()), dtype=torch.int16, device=self.device)
        clipped = np.zeros(len(entries), np.int64)
        for batch in self._batches(n, m, entries):
            src = torch.from_numpy(np.concatenate([sources[i] for i in batch])).to(self.device)
            src_len = n[batch]
            first, ids, snrs, starts, spans = [0], [], [], [], []
            for i in batch:
                for nid, snr, start, background in entries[i].noises:
                    k = self.noise_index[nid]
                    ids.append(k)
                    snrs.append(snr)
                    starts.append(start)
                    spans.append(-1 if background else int(self.noise_len[k]))
                first.append(len(ids))
            _, _, samples, clip, _ = ops.augment(
                self.cfg, src, exclusive_offsets(src_len), src_len, rir=self.rir_pool, rir_off=self.rir_off,
                rir_len=self.rir_len, rir_early=self.rir_early,
                utt_rir=[self.rir_index[entries[i].rir] if entries[i].rir is not None else -1 for i in batch], noise=self.noise_pool,
                noise_off=self.noise_off, noise_len=self.noise_len, nz_first=first, nz_id=ids, nz_snr=snrs, nz_start=starts, nz_span=spans,
                out_offsets=offsets[batch], out_pcm=pcm)
            assert np.array_equal(samples.cpu().numpy(), n_out[batch])
            clipped[batch] = clip.cpu().numpy()
        return pcm, offsets, n_out, clipped

    def augment(self, sources, entries):
        """The host convenience: ([int16 array per entry], clipped)."""
        pcm, offsets, lengths, clipped = self.run(sources, entries)
        host = pcm.cpu().numpy()
        return [host[o:o + k].copy() for o, k in zip(offsets, lengths)], clipped
