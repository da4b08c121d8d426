"""Sample-rate conversion and speed perturbation of waveforms on the GPU: the host side of xv_resample (include/xvector_hip.h), what the
`sox -r 8k` stages of the 8 kHz recipes (egs/sre/v1/local/make_musan.sh), compute-mfcc-feats --allow-downsample / --allow-upsample and
the 0.9 / 1.1 copies of x-vector training do.

    rs = Resampler(16000, 8000, "cuda:0")
    pcm, offsets, lengths, clipped = rs.run(waves)      # the packed int16 device tensor FeatureExtractor.extract_packed reads
    outs, clipped = rs.resample(waves)                  # int16 arrays
    fin, fout = speed_rates(0.9, 16000)                 # (14400, 16000): a speed factor F at rate fs is the resample F * fs -> fs

The arithmetic is Kaldi's LinearResample with ResampleWaveform's cutoff AS RESTATED in the header - not sox's resampler, and not `sox
speed`'s: DESIGN.md section 6f lists what is unpinned."""
from fractions import Fraction

import numpy as np

try:
    from .._host import DEFAULT_WORKSPACE_BYTES, device_ops, exclusive_offsets, greedy_batches
    from .waves import pack, unpack
except (ImportError, ValueError):
    from _host import DEFAULT_WORKSPACE_BYTES, device_ops, exclusive_offsets, greedy_batches
    from misc.waves import pack, unpack

SPEED_RANGE = (0.5, 2.0)


def _whole(value, what):
    """A rate given as a number or a decimal string as an exact whole number."""
    f = Fraction(repr(value) if isinstance(value, float) else str(value))
    if f.denominator != 1 or f < 1:
        raise ValueError("%s = %s Hz: a whole number of at least 1 is expected" % (what, value))
    return int(f)


def speed_rates(factor, sample_frequency):
    """(fin, fout) of the speed factor F at the rate fs: F * fs -> fs, F read as the decimal it is written as (0.9 is 9 / 10).  F * fs
    must be a whole number (0.9999 at 16 kHz is 15998.4: refused) and F must lie in 0.5 .. 2 and not be 1."""
    fs = _whole(sample_frequency, "the sample rate")
    try:
        f = Fraction(repr(factor) if isinstance(factor, float) else str(factor))
    except (ValueError, ZeroDivisionError):
        raise ValueError("speed=%s: a number is expected" % (factor,))
    if not SPEED_RANGE[0] <= f <= SPEED_RANGE[1] or f == 1:
        raise ValueError("speed=%s: a factor in %g .. %g other than 1 is expected" % (factor, SPEED_RANGE[0], SPEED_RANGE[1]))
    fin = f * fs
    if fin.denominator != 1:
        raise ValueError("speed=%s at %d Hz is a resample from %s Hz: speed * sample rate must be a whole number" % (factor, fs, float(fin)))
    return int(fin), fs


class Resampler(object):
    """Keeps the table of fin -> fout on the device and converts lists of waveforms in calls whose samples, in and out, stay within
    workspace_bytes."""

    def __init__(self, fin, fout, device="cuda:0", workspace_bytes=DEFAULT_WORKSPACE_BYTES, num_zeros=0, cutoff=0.0):
        self.torch, self.ops, self.device = device_ops(device)
        self.fin, self.fout = _whole(fin, "fin"), _whole(fout, "fout")
        self.cfg = self.ops.resample_config(self.fin, self.fout, num_zeros, cutoff)
        self.plan = self.ops.resample_plan(self.cfg)      # refuses equal rates and tables that do not fit, by name, before any GPU call
        self.tables = self.torch.from_numpy(self.ops.resample_tables(self.cfg)).to(self.device)
        self.workspace_bytes = int(workspace_bytes)

    def num_samples(self, n):
        return 0 if n <= 0 else (int(n) * self.plan["out_unit"] + self.plan["in_unit"] - 1) // self.plan["in_unit"]

    def _batches(self, n_in, n_out):
        grow = lambda i, total=0: (total + 2 * (n_in[i] + n_out[i]) + 32,)
        too_big = lambda i, cost: ("Resampler: a workspace of %d bytes does not hold utterance %d (%d samples in, %d out: %d bytes)"
                                   % (self.workspace_bytes, i, n_in[i], n_out[i], cost))
        return greedy_batches(len(n_in), grow, lambda total: total, self.workspace_bytes, max_items=65535, too_big=too_big)

    def run_packed(self, pcm, offsets, lengths):
        """Utterances that are on the device already: pcm an int16 device tensor, utterance i its samples offsets[i] .. offsets[i] +
        lengths[i] (host arrays) -> (pcm int16 device tensor, offsets int64 [b], lengths int64 [b], clipped int64 [b]), host arrays but for
        pcm: the converted utterances back to back, the layout ops.mfcc and ops.augment read."""
        offsets, lengths = np.asarray(offsets, np.int64).reshape(-1), np.asarray(lengths, np.int64).reshape(-1)
        n_out = np.asarray([self.num_samples(n) for n in lengths], np.int64)
        out_offsets = exclusive_offsets(n_out) if len(n_out) else np.zeros(0, np.int64)
        out = self.torch.empty(max(int(n_out.sum()), 1), dtype=self.torch.int16, device=self.device)
        clipped = np.zeros(len(lengths), np.int64)
        for j0 in range(0, len(lengths), 65535):
            j1 = min(j0 + 65535, len(lengths))
            _, _, samples, clip, _ = self.ops.resample(self.cfg, self.tables, pcm, offsets[j0:j1], lengths[j0:j1], out_offsets=out_offsets[j0:j1],
                                                       out_pcm=out)
            assert np.array_equal(samples.cpu().numpy(), n_out[j0:j1])
            clipped[j0:j1] = clip.cpu().numpy()
        return out, out_offsets, n_out, clipped

    def run(self, waves):
        """waves: int16 arrays -> (pcm int16 device tensor, offsets int64 [b], lengths int64 [b], clipped int64 [b]) as run_packed; the
        uploads are cut so that the samples of one call, in and out, stay within workspace_bytes."""
        torch = self.torch
        waves = [np.ascontiguousarray(w, dtype=np.int16).reshape(-1) for w in waves]
        n_in = [len(w) for w in waves]
        n_out = np.asarray([self.num_samples(n) for n in n_in], np.int64)
        out_offsets = exclusive_offsets(n_out) if waves else np.zeros(0, np.int64)
        out = torch.empty(max(int(n_out.sum()), 1), dtype=torch.int16, device=self.device)
        clipped = np.zeros(len(waves), np.int64)
        for batch in self._batches(n_in, n_out):
            src, offsets, n = pack([waves[i] for i in batch], self.device)
            if src is None:
                continue
            _, _, samples, clip, _ = self.ops.resample(self.cfg, self.tables, src, offsets, n, out_offsets=out_offsets[batch], out_pcm=out)
            assert np.array_equal(samples.cpu().numpy(), n_out[batch])
            clipped[batch] = clip.cpu().numpy()
        return out, out_offsets, n_out, clipped

    def resample(self, waves):
        """The host convenience: ([int16 array per waveform], clipped)."""
        pcm, offsets, lengths, clipped = self.run(waves)
        return unpack(pcm, offsets, lengths), clipped
