"""The bounds of tests/gemm16_ref.py held on the CPU before the kernels run: every row of tests/test_gpu_gemm16_forms.py with a plain
float32 NumPy evaluation of the same formulas (the planes of the model, three float32 products per block, float32 accumulation in the
form's block order) in place of the GPU must stay within its bound, equal float64 bit for bit on the position-coded operands, and leave
out no more than 1e-4 of its elements as mask-ambiguous.  Also: the plane model itself against its definition."""
import time

import numpy as np
import pytest

import bn_pool_ref as R
import gemm16_ref as S
import test_gpu_gemm16_forms as G

CPU = S.NumpyOps()


@pytest.fixture(scope="module", autouse=True)
def _ledger():
    t0 = time.time()
    yield
    G.write_ledger("float32 NumPy on the CPU", time.time() - t0)


# ------------------------------------------------------------------ the model
@pytest.mark.parametrize("amax,scale", [(1.0, 2.0 ** 12), (1.999, 2.0 ** 12), (2.0, 2.0 ** 11), (4095.9, 2.0), (4096.0, 1.0), (8191.0, 1.0), (8192.0, 0.5),
                                        (3e-4, 2.0 ** 24), (0.0, 1.0), (np.inf, 1.0), (1e-38, 2.0 ** 100), (3e38, 2.0 ** -100), (2.0 ** -88, 2.0 ** 100)])
def test_pow2_scale(amax, scale):
    """max |x| s in [2^12, 2^13) for every normal amax whose 12 - e lies within +-100; 1 for 0 and inf; the clamp beyond."""
    s = S.pow2_scale(S.bits_of(amax))
    assert s == np.float32(scale)
    if 0 < amax < np.inf and abs(np.log2(scale)) < 100:
        assert 2.0 ** 12 <= np.float32(amax) * s < 2.0 ** 13


def test_pow2_scale_of_nan_and_subnormal():
    assert S.pow2_scale(0x7fc00000) == 1 and S.pow2_scale(S.bits_of(1e-40)) == np.float32(2.0 ** 100)


def test_split_model_pieces():
    """h is x s to nearest even in 11 bits, l the remainder's rounding; subnormal low pieces are kept (quantum 2^-24); the pads are zero;
    h + l is within eps_rep of x s / s."""
    bits = S.bits_of(4096.0)      # s = 1
    x = np.array([[4096.0, 2049.0, 2051.0, 1.0 + 2.0 ** -11, 1.0 + 2.0 ** -10 + 2.0 ** -21, 2.0 ** -20, 3.0 * 2.0 ** -25, 2.0 ** -26, -2049.0, 0.0]], np.float32)
    h, l = S.plane_values(S.split(x, bits))
    assert h.shape == (1, 16) and np.all(h[:, 10:] == 0) and np.all(l[:, 10:] == 0)
    assert list(h[0, :10]) == [4096.0, 2048.0, 2052.0, 1.0, 1.0 + 2.0 ** -10, 2.0 ** -20, 4.0 * 2.0 ** -25, 0.0, -2048.0, 0.0]
    assert list(l[0, :10]) == [0.0, 1.0, -1.0, 2.0 ** -11, 2.0 ** -21, 0.0, 0.0, 0.0, -1.0, 0.0]      # (-2^-25, half a quantum, goes to -0)
    rs = np.random.RandomState(1)
    for scale in (1e-7, 1.0, 1e3):
        x = R.f32(rs.randn(37, 30) * scale)
        x[3, 5] = 1e4 * scale
        bits = S.amax_bits(x)
        h, l = S.plane_values(S.split(x, bits))
        assert np.all(np.abs(h) < 2.0 ** 13)
        rec = (R.f64(h) + R.f64(l))[:, :30] / float(S.pow2_scale(bits))
        assert np.all(np.abs(rec - x) <= S.eps_rep(x, bits))


def test_coded_operands_are_exact_in_any_order():
    for terms in (8, 160, 672, 3136):
        a, b = S.coded_wide((50, terms), terms, 1), S.coded_small((terms, 7), 2)
        assert np.abs(R.f64(a)).max() * 3 * terms <= 2 ** 23 and set(np.unique(b)) <= {-3.0, -2.0, -1.0, 1.0, 2.0, 3.0}
        h, l = S.plane_values(S.split(a, S.amax_bits(a)))
        assert np.array_equal(R.f64(h) + R.f64(l), R.f64(a) * float(S.pow2_scale(S.amax_bits(a))))
        _, lb = S.plane_values(S.split(b, S.amax_bits(b)))
        assert np.all(lb == 0) and (terms > 672 or np.any(l != 0))


def test_amax_model():
    assert S.amax_bits(np.array([0.5, -7.25, 3.0])) == S.bits_of(7.25)
    assert S.amax_bits(np.array([0.5]), S.bits_of(8.0)) == S.bits_of(8.0) and S.amax_bits(np.zeros(3)) == 0


def test_bn_apply_value_is_one_fused_operation():
    z, scale, shift = np.float32([[1.0 + 2.0 ** -12]]), np.float32([1.0 + 2.0 ** -12]), np.float32([-1.0])
    y = S.bn_apply_value(z, scale, shift, 0, None)
    assert y[0, 0] == np.float32(2.0 ** -11 + 2.0 ** -24) and (z * scale + shift)[0, 0] == np.float32(2.0 ** -11)      # the product alone rounds to even


# ------------------------------------------------------------------ the rows
@pytest.mark.parametrize("count", G.AMAX_CASES)
def test_amax_rows(count):
    G.row_amax(CPU, count)


@pytest.mark.parametrize("c", G.SPLIT_C)
@pytest.mark.parametrize("scale", [1e-7, 1.0, 1e3])
def test_split_planes_rows(c, scale):
    G.row_split_planes(CPU, c, scale)


@pytest.mark.parametrize("kind,n,pitched", G.BN_SPLIT_CASES)
def test_bn_apply_split_rows(kind, n, pitched):
    G.row_bn_apply_split(CPU, kind, n, pitched)


@pytest.mark.parametrize("row", G.FORWARD_ROWS, ids=[r["name"] for r in G.FORWARD_ROWS])
def test_nt_forward_bound(row):
    G.row_nt_forward(CPU, row)


@pytest.mark.parametrize("row", G.DGRAD_ROWS, ids=[r["name"] for r in G.DGRAD_ROWS])
def test_nt_dgrad_bound(row):
    G.row_nt_dgrad(CPU, row)


@pytest.mark.parametrize("segs,t_out,k,o,c", G.BWD_EPI_ROWS)
def test_nt_bwd_epilogue_bound(segs, t_out, k, o, c):
    G.row_nt_bwd_epilogue(CPU, segs, t_out, k, o, c)


@pytest.mark.parametrize("row", G.TN_ROWS, ids=[r["name"] for r in G.TN_ROWS])
def test_tn_bound(row):
    G.row_tn(CPU, row)


def test_rows_of_the_256_row_tiles_bound(monkeypatch):
    """The rows the child process of the GPU module runs under XV_CONV_WR=4, with the forms of that setting."""
    monkeypatch.setattr(G, "CONV_WR", 4)
    for row in G.FORWARD_ROWS_256:
        G.row_nt_forward(CPU, row)
    for row in G.DGRAD_ROWS_256:
        G.row_nt_dgrad(CPU, row)


def test_rows_cover_every_form():
    G.test_rows_cover_every_form()


def test_restatements_are_the_oracles_convolution():
    """spliced / weights_fwd / weights_dgrad (the layouts the backends hand the kernels) against the oracle in float64."""
    from oracle import xvector_oracle as O
    rs = np.random.RandomState(3)
    x, kern, bias, dz = (R.f64(v) for v in S.make_operands(rs, 3, 11, 5, 3, 6))
    ref = O.conv1d_valid_fwd(x, kern, bias).reshape(-1, 6)
    xp = np.zeros((3, 11, 8))
    xp[:, :, :5] = x
    assert np.allclose(S.spliced(xp, 3) @ R.f64(S.weights_fwd(R.f32(kern), 8)).T + bias, R.f64(S.forward(x, kern, bias)), rtol=1e-6, atol=1e-6)
    assert np.allclose(S.forward(x, kern, bias), ref, rtol=1e-12)
    dzp = np.zeros((3, 9 + 4, 8))
    dzp[:, 2:11, :6] = dz
    dx = S.spliced(dzp, 3) @ R.f64(S.weights_dgrad(R.f32(kern), 8)).T
    assert np.allclose(dx, S.dgrad(dz, kern, 11), rtol=1e-5, atol=1e-9)
    dk = np.einsum("rm,ro->mo", S.spliced(xp, 3), dz.reshape(-1, 6)).reshape(3, 8, 6)[:, :5]
    assert np.allclose(dk + 0.5 * kern, S.wgrad(x, dz, kern, 0.5), rtol=1e-10, atol=1e-12)
