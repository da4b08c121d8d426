"""The bounds of tests/segment_ref.py held on the CPU before the kernel runs: every row of tests/test_gpu_segment_forms.py with a plain
float32 NumPy evaluation of the same formulas in place of the GPU must stay within its bound, and no row may leave out more than 1e-4 of
its elements as mask-ambiguous.  Also: the BatchNorm restatements against the oracle's, in float64."""
import time

import numpy as np
import pytest

import bn_pool_ref as R
import segment_ref as S
import test_gpu_segment_forms as G
from oracle import xvector_oracle as O

CPU = S.NumpyOps()


@pytest.fixture(scope="module", autouse=True)
def _ledger():
    t0 = time.time()
    yield
    G.write_ledger("float32 NumPy on the CPU", time.time() - t0)


@pytest.mark.parametrize("shape,want,family", G.SPLIT_PARAMS)
def test_plain_splits_bound(shape, want, family):
    G.row_plain_splits(CPU, shape, want, family)


@pytest.mark.parametrize("with_bias,with_row,family", G.SHAPE_CASES)
def test_plain_shapes_bound(with_bias, with_row, family):
    G.row_plain_shapes(CPU, with_bias, with_row, family)


@pytest.mark.parametrize("family", ["base", "hetero"])
def test_plain_clamp_bound(family):
    G.row_plain_clamp(CPU, family)


@pytest.mark.parametrize("shape,kind,family", G.BN_FWD_CASES)
def test_bn_forward_bound(shape, kind, family):
    G.row_bn_forward(CPU, shape, kind, family)


@pytest.mark.parametrize("shape,kind,family", G.BN_BWD_CASES)
def test_bn_backward_bound(shape, kind, family):
    G.row_bn_backward(CPU, shape, kind, family)


@pytest.mark.parametrize("family", ["base", "hetero"])
def test_queue_is_the_launches_alone(family):
    G.row_ticket_hygiene(CPU, family)


@pytest.mark.parametrize("relu", [0, 1])
def test_restatements_are_the_oracles_batchnorm(relu):
    """S.bn_forward and S.bn_backward / S.bn_backward_dz in float64 against O.batchnorm_train_fwd / O.batchnorm_train_bwd on the same data."""
    rs = np.random.RandomState(11 + relu)
    m, n, k = 37, 12, 20
    x, wt, bias = (R.f64(v) for v in S.make_operands(rs, m, n, k, "hetero"))
    gamma, beta = (R.f64(v) for v in R.make_affine(rs, n, "hetero", negative=1))
    z = S.gemm(x, wt, bias)
    y, cache = O.batchnorm_train_fwd(z, gamma, beta, G.EPS)
    s = S.bn_forward(z, gamma, beta, np.float64(np.float32(G.EPS)), G.MOMENTUM, True, np.zeros(n), np.ones(n))
    assert np.allclose(s["mean"], cache[0], rtol=1e-12, atol=1e-300) and np.allclose(s["invstd"], cache[2], rtol=1e-6)      # (eps as a float32)
    assert np.allclose(z * s["scale"] + s["shift"], y, rtol=1e-6, atol=1e-9 * np.abs(y).max())
    mom, om = float(np.float32(G.MOMENTUM)), float(np.float32(1) - np.float32(G.MOMENTUM))
    assert np.allclose(s["moving_var"], mom + om * cache[1] * m / (m - 1.0), rtol=1e-9)
    # backward, on the oracle's own statistics so that the comparison is exact
    mean, invstd = cache[0], cache[2]
    scale = gamma * invstd
    shift = beta - mean * scale
    da = rs.randn(m, n)
    red = S.bn_backward(da, np.zeros((m, n)), z, gamma, mean, invstd, scale, shift, relu, None)
    dz, _ = S.bn_backward_dz(red, z, gamma, mean, invstd, red["dbeta"], red["dgamma"])
    dz_ref, dg_ref, db_ref = O.batchnorm_train_bwd(da * (y > 0) if relu else da, cache, gamma)
    for got, ref in ((red["dbeta"], db_ref), (red["dgamma"], dg_ref), (dz, dz_ref)):
        assert np.allclose(got, ref, rtol=1e-9, atol=1e-11 * np.abs(ref).max())
