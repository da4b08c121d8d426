"""The restatement of xv_resample (tests/resample_ref.py) against the figures the specification lists and against itself: the closed form
of the output length equals LinearResample's tick form, the weight rows sum to one within the window's ripple, a sine comes back."""
import numpy as np
import pytest

from tests import resample_ref as R

PAIRS = sorted(R.PAIRS)


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: "%d-%d" % p)
def test_units_taps_and_table_sizes_are_the_listed_figures(pair):
    plan = R.Plan(*pair)
    in_unit, out_unit, taps_min, taps_max, floats = R.PAIRS[pair]
    assert (plan.in_unit, plan.out_unit) == (in_unit, out_unit)
    assert (int(plan.taps.min()), int(plan.taps.max()), plan.taps_max) == (taps_min, taps_max, taps_max)
    assert plan.out_unit * plan.taps_max == floats == plan.w.size
    assert plan.table().size == 2 * out_unit + floats and plan.table().dtype == np.float32
    assert (plan.w[np.arange(taps_max)[None, :] >= plan.taps[:, None]] == 0.0).all()


def test_first_ranges_are_the_listed_figures():
    assert R.Plan(16000, 8000).first.tolist() == [-12]
    p = R.Plan(44100, 16000)
    assert (int(p.first.min()), int(p.first.max())) == (-16, 422)


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: "%d-%d" % p)
def test_closed_form_of_the_output_length_is_the_tick_form(pair):
    plan = R.Plan(*pair)
    for n in range(-1, 3 * plan.in_unit + 3):
        assert plan.num_samples(n) == plan.num_samples_ticks(n), n
    assert plan.num_samples(0) == 0 and plan.num_samples(-5) == 0 and plan.num_samples(1) == -(-plan.out_unit // plan.in_unit)


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: "%d-%d" % p)
def test_row_sums_lie_within_the_ripple(pair):
    sums = R.Plan(*pair).w.sum(axis=1)
    assert sums.min() >= 1.0000 and sums.max() <= 1.0010, (sums.min(), sums.max())


def test_speed_lengths():
    assert R.Plan(14400, 16000).num_samples(9000) == 10000 and R.Plan(14400, 16000).num_samples(9001) == 10002
    assert R.Plan(17600, 16000).num_samples(11000) == 10000 and R.Plan(17600, 16000).num_samples(11001) == 10001


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: "%d-%d" % p)
def test_a_sine_comes_back(pair):
    """440 Hz at amplitude 8000 is reproduced to within 3 away from the ends; the fp32 restatement stays beside the fp64 one.
    8000 -> 16000 is the one pair held to another figure: its interpolated phase has the largest row sum of the table, 1.00088 beside
    1.00004 for the phase that copies, a gain ripple of 8000 * 0.00088 = 7 at this amplitude, so its bound is amplitude * (largest row
    sum - 1) + 1 for the rounding of x (measured: 4.11; the six other pairs 0.90 .. 2.89)."""
    fin, fout = pair
    plan = R.Plan(fin, fout)
    n = int(0.05 * fin)
    x = np.round(8000.0 * np.sin(2 * np.pi * 440.0 * np.arange(n) / fin)).astype(np.int16)
    y = R.resample(x, plan)
    assert len(y) == plan.num_samples(n)
    want = 8000.0 * np.sin(2 * np.pi * 440.0 * np.arange(len(y)) / fout)
    edge = int(np.ceil(plan.ww * fout)) + 1
    bound = 3.0 if pair != (8000, 16000) else 8000.0 * (plan.w.sum(axis=1).max() - 1.0) + 1.0
    worst = np.abs(y - want)[edge:-edge].max()
    print("%d -> %d: a 440 Hz sine of amplitude 8000 comes back within %.2f (bound %.2f)" % (fin, fout, worst, bound))
    assert worst <= bound
    y32 = R.resample(x, plan, np.float32)
    assert y32.dtype == np.float32 and np.abs(y32 - y).max() <= plan.taps_max * 2.0 ** -24 * 8000.0 * 1.5


def test_a_full_scale_constant_clips_in_the_interior():
    """Row sum 1.00046 of 16000 -> 8000: 32767 becomes 32782, which the clamp changes."""
    plan = R.Plan(16000, 8000)
    y = R.resample(np.full(400, 32767, np.int16), plan)
    assert round(float(y[100])) == 32782
    pcm, clipped = R.quantise(y)
    assert clipped > 150 and pcm[100] == 32767


def test_quantise_rounds_to_nearest_even_then_clamps():
    pcm, clipped = R.quantise(np.array([0.5, 1.5, -0.5, -1.5, 2.4999, 32767.4, 32767.5, -32768.5, -32769.0]))
    assert pcm.tolist() == [0, 2, 0, -2, 2, 32767, 32767, -32768, -32768] and clipped == 2


def test_samples_outside_the_utterance_count_as_zero():
    plan = R.Plan(8000, 16000)
    x = np.array([1000], np.int16)
    d = {}
    y = R.resample(x, plan, details=d)
    assert len(y) == 2 and abs(y[0] - 1000 * plan.w[0, -plan.first[0]]) < 1e-9 and (d["magnitude"] >= np.abs(y) - 1e-9).all()
