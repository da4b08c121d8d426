"""The bounds of tests/bn_pool_ref.py held on the CPU before any kernel runs: every row of tests/test_gpu_bn_pool_forms.py with a plain
float32 NumPy evaluation of the same formulas in place of the GPU (NumPy's own summation order) must stay within its bound, and no row
may leave out more than 1e-4 of its elements as mask-ambiguous.  Also: the closed form of the restatement against the sums over z it
replaces, in float64 on exact pooled statistics."""
import time

import numpy as np
import pytest

import bn_pool_ref as R
import test_gpu_bn_pool_forms as G

CPU = R.NumpyOps()


@pytest.fixture(scope="module", autouse=True)
def _ledger():
    t0 = time.time()
    yield
    G.write_ledger("float32 NumPy on the CPU", time.time() - t0)


@pytest.mark.parametrize("rows,family", G.COL_STATS_CASES)
def test_col_stats_bound(rows, family):
    G.row_col_stats(CPU, rows, family)


@pytest.mark.parametrize("tiles,family", G.FINALIZE_CASES)
def test_bn_finalize_bound(tiles, family):
    G.row_bn_finalize(CPU, tiles, family)


@pytest.mark.parametrize("tiles,kind", G.OUTPUT_RANGE_CASES)
def test_bn_output_range_formula(tiles, kind):
    G.row_bn_output_range(CPU, tiles, kind)


@pytest.mark.parametrize("n", [1, 128, 129])
def test_bn_inference_scale_bound(n):
    G.row_bn_inference_scale(CPU, n)


@pytest.mark.parametrize("kind,pitched", G.APPLY_CASES)
def test_bn_apply_bound(kind, pitched):
    G.row_bn_apply(CPU, kind, pitched)


@pytest.mark.parametrize("kind,family", G.PLAIN_CASES)
def test_plain_backward_bound(kind, family):
    G.row_plain_backward(CPU, kind, family)


@pytest.mark.parametrize("kind", G.KINDS)
def test_plain_backward_second_trip_bound(kind):
    G.row_plain_backward(CPU, kind, "base", shapes=[(1, 16385, 0)], widths=(8,))


@pytest.mark.parametrize("kind,att,family", G.DIRECT_CASES)
def test_pooled_direct_bound(kind, att, family):
    G.row_pooled_direct(CPU, kind, att, family)


@pytest.mark.parametrize("relu,att,family", G.CLOSED_CASES)
def test_pooled_closed_bound(relu, att, family):
    G.row_pooled_closed(CPU, relu, att, family)


@pytest.mark.parametrize("kind,wmode,family", G.POOL_CASES)
def test_stat_pool_forward_bound(kind, wmode, family):
    G.row_stat_pool_forward(CPU, kind, wmode, family)


@pytest.mark.parametrize("b,t,c", G.POOL_BWD_CASES)
def test_stat_pool_backward_bound(b, t, c):
    G.row_stat_pool_backward(CPU, b, t, c)


@pytest.mark.parametrize("rows,n", G.L2_CASES)
def test_l2_scaling_bound(rows, n):
    G.row_l2_scaling(CPU, rows, n)


@pytest.mark.parametrize("relu,weighted", [(1, False), (1, True), (0, False), (0, True)])
def test_closed_form_is_the_sum_over_z_in_exact_arithmetic(relu, weighted):
    """R.closed_form on float64 pooled statistics of the very activation against R.bn_backward's sums: equal to float64 rounding, so what
    separates the two on float32 statistics is the statistics' own error (R.closed_form_residual)."""
    rs = np.random.RandomState(7 + relu + 2 * weighted)
    b, t, n = 5, 33, 8
    z, gamma, beta, dpool = G.pooled_inputs(rs, b, t, n, "hetero", special=True)
    w = G.frame_weights(rs, b, t, "random" if weighted else None)
    if weighted:
        w = R.f64(w) / R.f64(w).sum(axis=1, keepdims=True)      # the closed form takes the weights of a chunk to sum to 1
    s = R.bn_finalize(R.col_stats(z), b * t, gamma, beta, G.EPS, 0.99, False, None, None)
    vec = (s["mean"], s["invstd"], s["scale"], s["shift"])
    g64 = s["scale"] / s["invstd"]      # the gamma that scale and invstd imply
    mean_p, sd, wpos, _ = R.stat_pool_bn(z, b, t, s["scale"], s["shift"], relu, None, w)
    pool = np.concatenate([mean_p, sd], axis=1)
    red = R.bn_backward(z, g64, *vec, relu, None, 0, pooled=(pool, dpool, t, w))
    dbeta, dgamma, _, _ = R.closed_form(pool, dpool, wpos, g64, *vec, b * t)
    scale = np.abs(red["dd"]).sum(axis=0)
    assert np.all(np.abs(dbeta - red["dbeta"]) <= 1e-11 * scale)
    assert np.all(np.abs(dgamma - red["dgamma"]) <= 1e-9 * (np.abs(red["dd"] * red["xhat"]).sum(axis=0) + scale))
