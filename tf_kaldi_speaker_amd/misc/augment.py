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

from . import resample, waves
from .conf import _Options, _bool, _f, _i
from .features import DEFAULT_WORKSPACE_BYTES, _lib, device_ops, exclusive_offsets, greedy_batches
from .waves import read_scp, write_wav      # noqa: F401 (drivers and tests reach them here)

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


def read_signals(scp_path, sample_frequency, channel, what, resample_signals=False):
    """{id: int16 array} of a rir.scp / noise.scp style table: `id rxfilename` lines, RIFF PCM-16 at the sources' sample rate (without
    resample_signals there is no resampling; a mismatch is refused as by read_wav), `channel` of each file.  resample_signals: every rate
    passes and the table is {id: (int16 array, its rate in Hz)} - the Augmenter converts those that differ when it builds its pools."""
    opts = waves.WavFormat(sample_frequency, channel)
    out = {}
    for key, rx in read_scp(scp_path):
        if key in out:
            raise ValueError("%s: %s %s is listed twice" % (scp_path, what, key))
        samples, rate = waves.read_wav_rate(rx, opts, key, any_rate=bool(resample_signals))
        out[key] = (samples, rate) if resample_signals else samples
        if len(samples) == 0:
            raise ValueError("%s: %s %s holds no samples" % (scp_path, what, key))
    return out


def read_setup(options, rir_scp, noise_scp, sample_frequency, resample_signals=False, plan=""):
    """What a driver reads in front of an augmentation: -> (rirs, noises: the read_signals tables of rir.scp / noise.scp, each on its
    channel of options, {} for an empty path; the entries of the plan file checked against them, None for an empty path)."""
    rirs = read_signals(rir_scp, sample_frequency, options.impulse_response_channel, "impulse response", resample_signals) if rir_scp else {}
    noises = read_signals(noise_scp, sample_frequency, options.noise_channel, "noise", resample_signals) if noise_scp else {}
    return rirs, noises, (read_plan(plan, sample_frequency, rirs, noises) if plan else None)


class SourceError(ValueError):
    """A source of a plan entry that cannot be used: not listed, not readable, empty."""


def check_sources(entries, rx_of, plan_path, scp_path):
    """Refuses the first entry whose source is not a key of rx_of, the {key: rxfilename} of scp_path."""
    for e in entries:
        if e.src_key not in rx_of:
            raise SourceError("%s: Key %s: source %s is not in %s" % (plan_path, e.out_key, e.src_key, scp_path))


def plan_sources(entries, rx_of, options, plan_path, scp_path):
    """(entry, the samples of its source) per plan entry, in order: read by waves.read_wav under options as the entry is reached, once
    while consecutive entries name the same source.  SourceError: as check_sources, what read_wav refuses, a source without samples."""
    last = (None, None)
    for e in entries:
        check_sources([e], rx_of, plan_path, scp_path)
        if last[0] != e.src_key:
            try:
                last = (e.src_key, waves.read_wav(rx_of[e.src_key], options, e.src_key))
            except ValueError as err:
                raise SourceError(str(err))
        if len(last[1]) == 0:
            raise SourceError("Key %s: the source %s holds no samples" % (e.out_key, e.src_key))
        yield e, last[1]


def signal_seconds(signals, sample_frequency):
    """[(id, seconds)] of a read_signals table in either form (what make_plan takes)."""
    return [(k, len(v[0]) / float(v[1])) if isinstance(v, tuple) else (k, len(v) / float(sample_frequency)) for k, v in signals.items()]


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
        rirs, noises = self._at_rate(rirs or {}), self._at_rate(noises or {})
        self.rir_index, self.rir_pool, self.rir_off, self.rir_len = self._pool(rirs, "impulse response")
        self.noise_index, self.noise_pool, self.noise_off, self.noise_len = self._pool(noises, "noise")
        self.rir_early = [self.ops.augment_early(rirs[k], self.sample_frequency) for k in self.rir_index] if rirs else []

    def resampler(self, fin):
        """The Resampler fin -> sample_frequency of this Augmenter, kept: its table goes to the device once."""
        return waves.Resamplers.of(self)[fin, self.sample_frequency]

    def _at_rate(self, signals):
        """A read_signals table in either form as {id: int16 array at sample_frequency}: the (array, rate) entries whose rate differs are
        resampled on the device, once, grouped by rate (xv_resample; rounded to int16, as the wav of a `sox -r` stage is)."""
        out = {k: (v[0] if isinstance(v, tuple) else v) for k, v in signals.items()}
        keys = list(signals)
        groups = waves.by_rate(int(v[1]) if isinstance(v, tuple) and int(v[1]) != self.sample_frequency else None for v in signals.values())
        for rate, members in groups.items():
            converted, _ = self.resampler(rate).resample([out[keys[i]] for i in members])
            out.update(zip((keys[i] for i in members), converted))
        return out

    def perturbed(self, sources, entries):
        """The sources of the entries with speed=F resampled F * fs -> fs on the device, grouped by factor, and brought back as int16 (the
        intermediate a piped wav would be); the others as they are."""
        sources = list(sources)
        groups = waves.by_rate(None if e.speed is None else resample.speed_rates(e.speed, self.sample_frequency)[0] for e in entries)
        for fin, members in groups.items():
            converted, _ = self.resampler(fin).resample([sources[i] for i in members])
            for i, w in zip(members, converted):
                sources[i] = w
        return sources

    def _pool(self, signals, what):
        for k, a in signals.items():
            if np.size(a) == 0:
                raise ValueError("Augmenter: %s %s holds no samples" % (what, k))
        return ({k: i for i, k in enumerate(signals)},) + waves.pack(signals.values(), self.device)      # no signal: no pool (None)

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
            src, src_off, src_len = waves.pack([sources[i] for i in batch], self.device)
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
                self.cfg, src, src_off, src_len, rir=self.rir_pool, rir_off=self.rir_off,
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
        return waves.unpack(pcm, offsets, lengths), clipped
