"""tests/vlad_ref.py before a kernel runs (no GPU): the float64 restatement against the reference's own NumPy oracle
(tests/golden/vlad_golden.npz, model/test_utils.py:421-436), its backward against central differences, the zero residual, and the plain
float32 NumPy evaluation of every formula against the bounds the kernels are held to."""
import os

import numpy as np
import pytest

import vlad_ref as V

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vlad_golden.npz")


def test_restatement_matches_the_reference_oracle_at_float64_accuracy():
    g = np.load(GOLDEN)
    n = int(g["num_cases"])
    assert n == 6
    for i in range(n):
        value, key, cen, want = g["value_%d" % i], g["key_%d" % i], g["centers_%d" % i], g["vlad_%d" % i]
        k, final = int(g["num_centers_%d" % i]), bool(g["final_%d" % i])
        b, l, d = value.shape
        a = V.softmax(key.reshape(b * l, -1))
        r, _ = V.pool_forward(value, a, cen, k)
        got = V.normalize_forward(r, final)
        assert got.shape == want.shape == (b, k * d)
        # both sides are float64 evaluations of the same sums in another order; the epsilon never binds here (|R|^2 >> 1e-12)
        assert np.abs(got - want).max() <= 64 * 2.0 ** -53 * max(1.0, np.abs(want).max()), i


def _loss(x, w, bias, cen, k, final, proj):
    out, _ = V.vlad_forward(x, w, bias, cen, k, final)
    return float((out * proj).sum())


@pytest.mark.parametrize("final", [False, True])
@pytest.mark.parametrize("shape", [(2, 5, 8, 3, 2), (3, 4, 4, 1, 0), (1, 1, 8, 2, 1)])
def test_backward_matches_central_differences(shape, final):
    b, t, c, k, g = shape
    rs = np.random.RandomState(7 + b + 10 * t)
    x, w, bias, cen = (V.f64(v) for v in V.make_case(rs, b, t, c, k, g))
    proj = rs.randn(b, k * c)
    out, cache = V.vlad_forward(x, w, bias, cen, k, final)
    dx, dw, db, dc = V.vlad_backward(proj, cache)
    h = 1e-6
    for name, arr, grad in (("x", x, dx), ("w", w, dw), ("bias", bias, db), ("centers", cen, dc)):
        num = np.zeros_like(arr)
        it = np.nditer(arr, flags=["multi_index"])
        for _ in it:
            idx = it.multi_index
            keep = arr[idx]
            arr[idx] = keep + h
            up = _loss(x, w, bias, cen, k, final, proj)
            arr[idx] = keep - h
            dn = _loss(x, w, bias, cen, k, final, proj)
            arr[idx] = keep
            num[idx] = (up - dn) / (2 * h)
        # central differences in float64: truncation h^2 |f'''| and rounding 2^-53 |f| / h, both ~1e-10 of the gradient's scale
        assert np.abs(num - grad).max() <= 1e-6 * max(1.0, np.abs(grad).max()), (name, np.abs(num - grad).max())
    assert np.allclose(dc[k:], 0.0) and np.allclose(db.sum(), 0.0, atol=1e-12)      # ghosts: softmax only; the softmax's gradients sum to 0


def test_regulariser_covers_the_kernel_and_every_centre_not_the_bias():
    rs = np.random.RandomState(3)
    x, w, bias, cen = (V.f64(v) for v in V.make_case(rs, 2, 3, 4, 2, 1))
    out, cache = V.vlad_forward(x, w, bias, cen, 2, False)
    g0 = V.vlad_backward(np.zeros_like(out), cache, l2=0.0)
    g1 = V.vlad_backward(np.zeros_like(out), cache, l2=0.5)
    assert np.allclose(g1[1] - g0[1], 0.5 * w) and np.allclose(g1[3] - g0[3], 0.5 * cen) and np.allclose(g1[2], g0[2])


@pytest.mark.parametrize("final", [False, True])
@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_zero_residual_gives_zero_and_finite_gradients(dt, final):
    """Every frame equals every centre: the residuals are exactly 0, the output is 0 (not NaN: the epsilon), and the gradient passes through
    the clamped norm as the constant 1 / sqrt(eps)."""
    b, t, c, k, g = 2, 5, 8, 2, 1
    rs = np.random.RandomState(5)
    cen = np.tile(V.f32(rs.rand(c)), (k + g, 1))
    x = np.tile(cen[0], (b, t, 1))
    w, bias = V.f32(rs.randn(c, k + g) * 0.1), V.f32(rs.randn(k + g) * 0.1)
    out, cache = V.vlad_forward(x, w, bias, cen, k, final, dt=dt)
    assert np.all(out == 0)
    grads = V.vlad_backward(np.ones_like(out), cache, dt=dt)
    for gr in grads:
        assert np.all(np.isfinite(gr))
    scale = 1e6 * (1e6 if final else 1.0)
    assert np.allclose(V.normalize_backward(cache["r"], np.ones_like(out), final, dt), scale, rtol=1e-5)


def test_float32_numpy_evaluation_is_inside_every_bound():
    """The bounds are statements about float32 arithmetic: the plain NumPy float32 evaluation must satisfy them as well."""
    rs = np.random.RandomState(11)
    for (b, t, c, k, g, hostile) in ((3, 9, 8, 3, 2, False), (4, 7, 1500, 10, 2, True), (1, 200, 8, 17, 3, False)):
        x, w, bias, cen = V.make_case(rs, b, t, c, k, g, hostile)
        logits = V.f32(V.f64(x).reshape(b * t, c) @ V.f64(w) + V.f64(bias))
        a32 = V.f32(V.softmax(logits, np.float32))
        assert np.all(np.abs(a32 - V.softmax(logits)) <= V.softmax_bound(logits))
        r64, n64 = V.pool_forward(x, a32, cen, k)
        r32, n32 = V.pool_forward(x, a32, cen, k, dt=np.float32)
        br, bn = V.pool_forward_bound(x, a32, cen, k, chain=max(t - 1, V.cdiv(t, 4) + 3))      # NumPy adds the t frames in its own order
        assert np.all(np.abs(r32 - r64) <= br) and np.all(np.abs(n32 - n64) <= bn)
        r = V.f32(r64)
        for final in (False, True):
            assert np.all(np.abs(V.normalize_forward(r, final, np.float32) - V.normalize_forward(r, final)) <= V.normalize_forward_bound(r, final))
        dr = V.f32(rs.randn(b, k, c))
        da64, dx64 = V.pool_backward(x, a32, cen, dr)
        da32, dx32 = V.pool_backward(x, a32, cen, dr, np.float32)
        bda, bdx = V.pool_backward_bound(x, a32, cen, dr, chain=max(c - 1, V.row_chain(c)))
        assert np.all(np.abs(da32 - da64) <= bda) and np.all(np.abs(dx32 - dx64) <= bdx)
        da = V.f32(da64)
        assert np.all(np.abs(V.softmax_backward(a32, da, np.float32) - V.softmax_backward(a32, da)) <= V.softmax_backward_bound(a32, da))
        n = V.f32(n64)
        assert np.all(np.abs(V.centers_backward(n, dr, cen, 0.01, np.float32) - V.centers_backward(n, dr, cen, 0.01))
                      <= V.centers_backward_bound(n, dr, cen, 0.01, chain=b + 16))


def test_ragged_lengths_pool_the_valid_rows_only():
    rs = np.random.RandomState(2)
    x, w, bias, cen = V.make_case(rs, 3, 9, 8, 2, 1)
    a = V.softmax(V.f64(x).reshape(27, 8) @ V.f64(w) + V.f64(bias))
    frames, shrink = np.array([23, 18, 40]), 14      # 9, 4 and (clamped) 9 rows
    r, n = V.pool_forward(x, a, cen, 2, frames, shrink)
    for i, tv in enumerate((9, 4, 9)):
        ri, ni = V.pool_forward(x[i:i + 1, :tv], a.reshape(3, 9, 3)[i, :tv], cen, 2)
        assert np.allclose(r[i], ri[0], rtol=0, atol=1e-14) and np.allclose(n[i], ni[0], rtol=0, atol=1e-14)
