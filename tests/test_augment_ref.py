"""The restatement of xv_augment (tests/augment_ref.py) against independent evaluations of its rules: the convolution against
scipy.signal.fftconvolve and a three-tap case worked by hand, E / g_j / the scale against their formulas on a toy case, the background span
against np.tile, shift and wrap, truncate and clamp at the edges.  No GPU."""
import numpy as np
import pytest

from tests import augment_ref as A


def test_convolution_by_hand_and_against_fftconvolve():
    # x = [1, 2, 3], h = [4, -5, 6]: y[0] = 4, y[1] = 8 - 5 = 3, y[2] = 12 - 10 + 6 = 8, y[3] = -15 + 12 = -3, y[4] = 18
    want = np.array([4.0, 3.0, 8.0, -3.0, 18.0])
    x, h = np.array([1, 2, 3], np.int16), np.array([4, -5, 6], np.int16)
    assert np.array_equal(A.conv64(x, h), want)
    for kb in (1, 2, 3, 32):
        got = A.conv32(x, h, kb)
        assert got.dtype == np.float32 and np.array_equal(got, want)
    from scipy.signal import fftconvolve
    rs = np.random.RandomState(3)
    x, h = A.signal(rs, 700), A.rir(rs, 133, 37)
    ref = fftconvolve(x.astype(np.float64), h.astype(np.float64))
    y64 = A.conv64(x, h)
    assert y64.shape == ref.shape == (832,)
    assert np.abs(y64 - ref).max() <= 1e-9 * np.abs(ref).max()
    assert np.array_equal(y64, np.round(y64))                       # whole numbers: the fp64 form is exact
    for kb in (7, 32):
        y32 = A.conv32(x, h, kb)
        bound = (kb + -(-133 // kb)) * 2.0 ** -24 * np.convolve(np.abs(x.astype(np.float64)), np.abs(h.astype(np.float64)))
        assert (np.abs(y32 - y64) <= bound).all() and np.abs(y32 - y64).max() > 0


def test_energy_gain_and_scale_against_their_formulas():
    fs = 16000.0
    rs = np.random.RandomState(5)
    x, h, v = A.signal(rs, 900), A.rir(rs, 1200, 40), A.signal(rs, 300)
    es, ee, p = A.early(h, fs)
    assert (es, ee, p) == (40 - 16, 40 + 800, 40)
    assert A.early(A.rir(rs, 60, 3), fs) == (0, 60, 3)               # both ends cut
    d = {}
    out = A.augment(x, h, [(v, 10.0, 100, None)], fs=fs, shift_output=0, normalize_output=1, volume=0.5, details=d)
    xd, vd = x.astype(np.float64), v.astype(np.float64)
    P0 = np.mean(xd ** 2)
    e = np.convolve(xd, h[es:ee].astype(np.float64))
    E = np.sum(e ** 2) / (900 + (ee - es) - 1)
    g = np.sqrt(10.0 ** -1.0 * E / np.mean(vd ** 2))
    y = np.convolve(xd, h.astype(np.float64))
    y[100:400] += g * vd
    s = np.sqrt(P0 / np.mean(y ** 2)) * 0.5
    assert d["M"] == 900 + 1200 - 1 == len(out) and d["p"] == 40
    assert np.isclose(d["P0"], P0, rtol=1e-14) and np.isclose(d["E"], E, rtol=1e-14)
    assert np.isclose(d["gains"][0], g, rtol=1e-14) and np.isclose(d["scale"], s, rtol=1e-14)
    assert np.allclose(out, y * s, rtol=1e-13, atol=0)
    assert np.isclose(np.mean(out ** 2), 0.25 * P0, rtol=1e-12)      # normalised to the source's power, then the volume
    # without an impulse response E is the source's power; a silent noise and one that starts behind the end add nothing
    d2 = {}
    out2 = A.augment(x, None, [(np.zeros(50, np.int16), 0.0, 0, None), (v, 0.0, 900, None), (v, 5.0, 850, None)], normalize_output=0, details=d2)
    assert d2["E"] == d2["P0"] and d2["gains"][:2] == [0.0, 0.0] and d2["scale"] == 1.0
    assert np.array_equal(out2[:850], xd[:850]) and np.allclose(out2[850:], xd[850:] + d2["gains"][2] * vd[:50], rtol=1e-14)
    # the fp32 form stays close, and is fp32
    o32 = A.augment(x, h, [(v, 10.0, 100, None)], fs=fs, shift_output=0, volume=0.5, dtype=np.float32)
    assert o32.dtype == np.float32 and 0 < np.abs(o32 - out).max() < 1e-5 * np.abs(out).max()


def test_background_span_is_the_noise_tiled():
    rs = np.random.RandomState(7)
    x, v = A.signal(rs, 1000), A.signal(rs, 300)
    assert np.array_equal(A.noise_signal(v, 1000), np.tile(v, 4)[:1000])
    d = {}
    out = A.augment(x, None, [(v, 8.0, 0, "bg")], normalize_output=0, details=d)
    t = np.tile(v, 4)[:1000].astype(np.float64)
    g = np.sqrt(10.0 ** -0.8 * d["P0"] / np.mean(t ** 2))              # the power of the SPAN, not of the noise file
    assert np.isclose(d["gains"][0], g, rtol=1e-14) and np.allclose(out, x + g * t, rtol=1e-14)
    assert not np.isclose(np.mean(t ** 2), np.mean(v.astype(np.float64) ** 2), rtol=1e-6)


def test_shift_and_wrap():
    x, h = np.array([100, 200, 300, 400], np.int16), np.array([1, 2, 10, 3], np.int16)      # peak at 2, M = 7
    y = np.convolve(x.astype(np.float64), h.astype(np.float64))
    full = A.augment(x, h, normalize_output=0, shift_output=0)
    assert np.array_equal(full, y) and len(full) == 7
    cut = A.augment(x, h, normalize_output=0, shift_output=1)
    assert np.array_equal(cut, y[2:6])                                   # out[i] = y[i + p], n samples
    # the wrap: i + p <= (n - 1) + (L - 1) = M - 1, so with shift = p < L the mod of step 6 never folds; the index rule is what is held
    d = {}
    A.augment(x, h, normalize_output=0, details=d)
    assert d["M"] == 7 and d["p"] == 2
    idx = (np.arange(4) + 2) % 7
    assert np.array_equal(cut, y[idx])
    one = A.augment(x, np.array([7], np.int16), normalize_output=0)
    assert np.array_equal(one, 7.0 * x)


@pytest.mark.parametrize("v, want, clipped", [(0.5, 0, 0), (-0.5, 0, 0), (0.999, 0, 0), (-0.999, 0, 0), (1.0, 1, 0), (-1.999, -1, 0),
                                              (32767.5, 32767, 0), (-32767.5, -32767, 0), (32768.0, 32767, 1), (-32768.9, -32768, 0),
                                              (-32769.0, -32768, 1), (1e9, 32767, 1)])
def test_truncate_then_clamp(v, want, clipped):
    q, c = A.quantise(np.array([v]))
    assert q.dtype == np.int16 and int(q[0]) == want and c == clipped


def test_generators():
    rs = np.random.RandomState(11)
    for n in (1, 5, 4000):
        x = A.signal(rs, n)
        assert x.dtype == np.int16 and len(x) == n and np.abs(x.astype(np.int32)).max() <= 8000 and x.any()
    for L, peak in ((1, 0), (2, 1), (33, 0), (33, 32), (4001, 37)):
        h = A.rir(rs, L, peak)
        assert h.dtype == np.int16 and len(h) == L and A.early(h)[2] == peak and h[0] != 0 and abs(int(h[-1])) >= 1500
