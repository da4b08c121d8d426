"""CPU checks of the NumPy restatement of VBx (tests/vbx_ref.py), the checker of tests/test_gpu_vbx.py: the log-domain definition against
the per-frame scaled form the kernel computes, the ELBO's monotony, the edge cases, vbx_init, and the conditioning of the shared inputs."""
import numpy as np
import pytest

from tests import vbx_ref as R
from tf_kaldi_speaker_amd.misc.diarization import VbxOptions, vbx_init


@pytest.mark.parametrize("params", R.PARAMS)
@pytest.mark.parametrize("shape", R.SHAPES)
def test_log_domain_and_scaled_forms_agree_in_float64(shape, params):
    """Measured worst cases over the shapes and both parameter sets, one iteration from the shared start (all at 2048 x 256 x 32 under
    (1, 1, 0.9)): gamma 2.0e-8, pi 2.9e-10, ELBO 7.9e-15 relative; 65 x 8 x 4: gamma 9.4e-13.  The log-domain form itself loses that much at
    T = 2048: its forward variable reaches -8e5, where a float64 ulp is 1.2e-10.  Asserted: the measured worst case times 8."""
    c, (fa, fb, lp) = R.case(shape), params
    gl, pl, el, tl, sl = R.iteration_log(c["x"], c["phi"], c["gamma"], c["pi"], lp, fa, fb)
    gs, ps, es, ts, ss = R.one_iteration(shape, params, np.float64)
    assert np.abs(gl - gs).max() <= 8 * 2.0e-8 and np.abs(pl - ps).max() <= 8 * 2.9e-10
    assert abs(el - es) <= 8 * 7.9e-15 * abs(el) and ss == sl
    for g, p, tol in ((gl, pl, 8 * 2.0e-8), (gs, ps, 1e-12)):      # (the log-domain rows carry that form's own loss)
        assert np.abs(g.sum(axis=1) - 1).max() < tol and abs(p.sum() - 1) < 1e-12 and g.min() >= 0 and p.min() >= 0


@pytest.mark.parametrize("shape", R.SHAPES)
def test_float32_scaled_form_is_usable(shape):
    """The scaled form in float32 stays close to float64 after one iteration (the naive log-domain recursion in float32 does not):
    measured worst over the shapes and parameter sets gamma 1.4e-4, pi 4.4e-6, ELBO 1.3e-6 relative."""
    for params in R.PARAMS:
        g3, p3, e3 = R.one_iteration(shape, params, np.float32)[:3]
        g6, p6, e6 = R.one_iteration(shape, params, np.float64)[:3]
        assert g3.dtype == np.float32 and p3.dtype == np.float32
        assert np.abs(g3 - g6).max() <= 9e-4 and np.abs(p3 - p6).max() <= 5e-5 and abs(e3 - e6) <= 2e-6 * abs(e6)
        # (the backward variable carries one rounding per frame into the rows' sums: at most (T + S) ulps of 1; observed 1.4e-5 at T = 2048)
        assert np.abs(g3.sum(axis=1) - 1).max() < (shape[0] + shape[2]) * 2.0 ** -23 and abs(float(p3.sum()) - 1) < 1e-6


@pytest.mark.parametrize("shape", R.SHAPES)
def test_elbo_never_falls_and_the_inputs_are_well_conditioned(shape):
    """20 float64 iterations under (0.3, 17, 0.99): the ELBO never falls by more than 1e-12 |ELBO| (observed worst: 2.9e-16 relative), the
    run ends with the true number of speakers, purity 1 and - for the seed the GPU tests use - a gap of at least 0.5 between the two
    largest responsibilities of every row (observed: 0.508 at 65 x 8 x 4 seed 2, >= 0.95 everywhere else)."""
    seed = R.gap_checked_seed(shape)
    assert seed == 0
    g, labels, elbos = R.converged(shape, seed)
    e = np.asarray(elbos)
    assert len(e) == 20 and (np.diff(e) >= -1e-12 * np.abs(e[1:])).all()
    assert R.row_gap(g) >= 0.5
    who = R.case(shape, seed)["who"]
    assert np.array_equal(R.first_appearance(labels), R.first_appearance(who))
    assert np.abs(g.sum(axis=1) - 1).max() < 1e-12


def test_stop_rule():
    c, (fa, fb, lp) = R.case((65, 8, 4)), R.PARAMS[0]
    full = R.converged((65, 8, 4), 0)[2]
    gains = np.diff(full)
    eps = 0.5 * (gains[2] + gains[3]) if gains[3] < gains[2] else gains[2] * 0.5
    first = 1 + int(np.argmax(gains < eps))
    elbos = R.vbx(c["x"], c["phi"], c["gamma"], c["pi"], lp, fa, fb, 20, eps, "scaled", np.float64)[2]
    assert len(elbos) == first + 1 < 20 and elbos == full[:first + 1]
    assert len(R.vbx(c["x"], c["phi"], c["gamma"], c["pi"], lp, fa, fb, 1, np.inf)[2]) == 1      # the first iteration never stops on the rule


def test_one_row_and_one_speaker():
    for form in (R.iteration_log, R.iteration_scaled):
        rs = np.random.RandomState(3)
        x, phi = rs.randn(1, 4), np.linspace(8, 0.1, 4)
        pi = np.array([0.2, 0.5, 0.3])
        g, p, e = form(x, phi, np.array([[0.6, 0.3, 0.1]]), pi, 0.9, 0.3, 17.0)[:3]
        assert g.shape == (1, 3) and np.allclose(g.sum(), 1) and np.allclose(p, g[0]) and np.isfinite(e)      # T = 1: gamma_0 ~ pi * p_0, pi <- gamma_0
        x = rs.randn(9, 4)
        g, p, e = form(x, phi, np.ones((9, 1)), np.ones(1), 0.9, 0.3, 17.0)[:3]
        assert np.allclose(g, 1) and np.allclose(p, 1) and np.isfinite(e)                                      # S = 1
    a = R.iteration_log(x, phi, np.ones((9, 1)), np.ones(1), 0.9, 0.3, 17.0)
    b = R.iteration_scaled(x, phi, np.ones((9, 1)), np.ones(1), 0.9, 0.3, 17.0, np.float64)
    assert abs(a[2] - b[2]) < 1e-12 * abs(a[2])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_dead_speaker_stays_dead(dtype):
    c = R.case((65, 8, 4))
    pi = np.array([0.5, 0.0, 0.25, 0.25])
    gamma = c["gamma"].astype(np.float64).copy()
    gamma[:, 1] = 0
    gamma /= gamma.sum(axis=1, keepdims=True)
    x = c["x"].copy()
    x[7] *= 40.0      # a row far from every live model: the dead speaker's flat model scores best there by far
    for _ in range(3):
        gamma, pi, e = R.iteration_scaled(x, c["phi"], gamma, pi, 0.99, 0.3, 17.0, dtype)[:3]
        assert np.isfinite(gamma).all() and np.isfinite(pi).all() and np.isfinite(e)
        assert (gamma[:, 1] == 0).all() and pi[1] == 0 and abs(float(pi.sum()) - 1) < 1e-6
    g64 = R.iteration_log(x, c["phi"], c["gamma"], np.array([0.5, 0.0, 0.25, 0.25]), 0.99, 0.3, 17.0)[0]
    assert np.isfinite(g64).all() and (g64[:, 1] == 0).all()


def test_vbx_init():
    g = vbx_init([0, 2, 2, 1], 3, 5.0)
    assert g.dtype == np.float32 and g.shape == (4, 3) and np.abs(g.sum(axis=1) - 1).max() < 1e-6
    e5 = np.exp(5.0)
    assert np.allclose(g[0], [e5 / (e5 + 2), 1 / (e5 + 2), 1 / (e5 + 2)]) and g[1].argmax() == 2 and g[3].argmax() == 1
    assert np.allclose(vbx_init([0, 1], 2, 0.0), 0.5) and (vbx_init([0, 0], 1) == 1).all()
    for bad in (([0, 3], 3), ([-1], 2), ([], 2), ([[0]], 2)):
        with pytest.raises(ValueError, match="vbx_init: labels must be"):
            vbx_init(*bad)
    with pytest.raises(ValueError, match="smoothing must not be negative"):
        vbx_init([0], 1, -1.0)
    o = VbxOptions()
    assert (o.fa, o.fb, o.loop_prob, o.max_iters, o.epsilon, o.init_smoothing) == (0.3, 17.0, 0.99, 20, 1e-4, 5.0)


def test_generator():
    c = R.case((130, 16, 6))
    assert c["x"].shape == (130, 16) and c["x"].dtype == np.float32 and c["gamma"].shape == (130, 6) and c["pi"].shape == (6,)
    assert np.allclose(c["phi"], np.linspace(8, 0.1, 16)) and len(np.unique(c["who"])) == 3
    runs = np.diff(np.flatnonzero(np.concatenate([[1], np.diff(c["who"]) != 0, [1]])))
    assert runs[:-1].min() >= 6      # turns of 6 to 23 windows (two turns of one speaker may abut; the last one is cut by T)
    start = c["gamma"].argmax(axis=1)
    assert 0.8 <= np.mean(start // 2 == c["who"]) < 1.0 and len(np.unique(start)) > 3      # split in two, 10 % random labels
