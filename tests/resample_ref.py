"""NumPy restatement of xv_resample (include/xvector_hip.h): Kaldi's LinearResample with ResampleWaveform's cutoff as this project restates
it.  Kaldi is not available where the tests run, so this is parity BY RESTATEMENT: the header states the rules, this module restates them,
the kernel is held against it.  resample(..., dtype=np.float64) is the reference: the table in double, every sum in double.
dtype=np.float32 follows the kernel's number format and order - the table rounded to fp32 once, one sequential chain of fused
multiply-adds from zero in increasing j per output - and measures what the format alone costs: the GPU tests derive their tolerance from
the distance between the two.  An fma of an fp32 weight and an int16-valued sample is formed in double (the product is exact there) and
rounded once."""
from math import gcd

import numpy as np

# the pairs of the issue's table: (fin, fout) -> (in_unit, out_unit, taps_min, taps_max, table floats)
PAIRS = {(16000, 8000): (2, 1, 25, 25, 25), (8000, 16000): (1, 2, 12, 13, 26), (14400, 16000): (9, 10, 12, 13, 130),
         (17600, 16000): (11, 10, 13, 14, 140), (44100, 16000): (441, 160, 33, 34, 5440), (44100, 8000): (441, 80, 66, 67, 5360),
         (16000, 11025): (640, 441, 17, 18, 7938)}


class Plan(object):
    """The units, first[], taps[] and the weight rows w [out_unit, taps_max] (float64) of fin -> fout."""

    def __init__(self, fin, fout, num_zeros=6, cutoff=None):
        assert fin != fout and fin >= 1 and fout >= 1
        self.fin, self.fout, self.num_zeros = int(fin), int(fout), int(num_zeros)
        self.cutoff = 0.99 * 0.5 * min(fin, fout) if cutoff is None else float(cutoff)
        g = gcd(self.fin, self.fout)
        self.in_unit, self.out_unit = self.fin // g, self.fout // g
        self.ww = self.num_zeros / (2.0 * self.cutoff)
        t = np.arange(self.out_unit, dtype=np.float64) / float(self.fout)
        self.first = np.ceil((t - self.ww) * self.fin).astype(np.int64)
        last = np.floor((t + self.ww) * self.fin).astype(np.int64)
        self.taps = last - self.first + 1
        self.taps_max = int(self.taps.max())
        j = np.arange(self.taps_max, dtype=np.int64)
        k = self.first[:, None] + j[None, :]
        d = k / float(self.fin) - t[:, None]
        window = np.where(np.abs(d) < self.ww, 0.5 * (1.0 + np.cos(2.0 * np.pi * self.cutoff / self.num_zeros * d)), 0.0)
        safe = np.where(d != 0.0, d, 1.0)
        filt = np.where(d != 0.0, np.sin(2.0 * np.pi * self.cutoff * d) / (np.pi * safe), 2.0 * self.cutoff)
        self.w = np.where(j[None, :] < self.taps[:, None], filt * window / self.fin, 0.0)

    def table(self):
        """The layout of xv_resample_tables: first, taps (whole numbers as floats), the rows - float32."""
        return np.concatenate([self.first.astype(np.float32), self.taps.astype(np.float32), self.w.astype(np.float32).reshape(-1)])

    def num_samples(self, n):
        """The closed form: ceil(n * out_unit / in_unit) in whole numbers."""
        return 0 if n <= 0 else (int(n) * self.out_unit + self.in_unit - 1) // self.in_unit

    def num_samples_ticks(self, n):
        """LinearResample::GetNumOutputSamples with flush = true, in ticks of 1 / lcm(fin, fout) seconds."""
        if n <= 0:
            return 0
        tick_freq = self.fin // gcd(self.fin, self.fout) * self.fout
        ticks_per_input = tick_freq // self.fin
        interval = int(n) * ticks_per_input
        ticks_per_output = tick_freq // self.fout
        last = interval // ticks_per_output
        if last * ticks_per_output == interval:
            last -= 1
        return last + 1


def _fma32(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def resample(x, plan, dtype=np.float64, details=None):
    """x: int16 array -> the n_out samples of y in `dtype`, not quantised.  details: a dict that receives `magnitude` = sum_j |w| |x| per
    output (the derived bound's)."""
    x = np.asarray(x)
    n = len(x)
    n_out = plan.num_samples(n)
    f32 = dtype == np.float32
    w = plan.w.astype(np.float32) if f32 else plan.w
    o = np.arange(n_out, dtype=np.int64)
    q, i = o // plan.out_unit, o % plan.out_unit
    f = plan.first[i] + q * plan.in_unit
    xd = x.astype(np.float64)
    y = np.zeros(n_out, dtype)
    mag = np.zeros(n_out, np.float64)
    for j in range(plan.taps_max):
        k = f + j
        inside = (k >= 0) & (k < n)
        xv = np.where(inside, xd[np.clip(k, 0, max(n - 1, 0))], 0.0) if n else np.zeros(n_out)
        wj = w[i, j]
        y = _fma32(wj, xv, y) if f32 else y + wj * xv
        if details is not None:
            mag += np.abs(wj.astype(np.float64)) * np.abs(xv)
    if details is not None:
        details["magnitude"] = mag
    return y


def quantise(v):
    """PCM-16: round to nearest, ties to even, then clamp -> (int16, how many samples the clamp changed)."""
    r = np.rint(np.asarray(v, np.float64))
    c = np.clip(r, -32768.0, 32767.0)
    return c.astype(np.int16), int((c != r).sum())


def signal(rs, n, fs=16000.0, peak=20000):
    """n int16 samples of peak <= `peak`: a sine plus noise."""
    t = np.arange(n, dtype=np.float64) / fs
    x = 0.6 * peak * np.sin(2 * np.pi * rs.uniform(200.0, 0.2 * fs) * t + rs.uniform(0, 6.28)) + 0.1 * peak * rs.randn(n)
    return np.clip(np.round(x), -peak, peak).astype(np.int16)
