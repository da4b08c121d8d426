"""The bounds of tests/attention_ref.py held on the CPU before any kernel runs: every row of tests/test_gpu_attention_forms.py with a plain
float32 NumPy evaluation of the same formulas in place of the GPU must stay within its bound, and no row may leave out more than 1e-4 of
its elements as mask-ambiguous.  Also: the restatements against the oracle's self-attention forward and backward, in float64."""
import time

import numpy as np
import pytest

import attention_ref as A
import bn_pool_ref as R
import test_gpu_attention_forms as G
from oracle import xvector_oracle as O

CPU = A.NumpyOps()


@pytest.fixture(scope="module", autouse=True)
def _ledger():
    t0 = time.time()
    yield
    G.write_ledger("float32 NumPy on the CPU", time.time() - t0)


@pytest.mark.parametrize("act,family", G.SCORE_CASES)
def test_att_score_bound(act, family):
    G.row_att_score(CPU, act, family)


@pytest.mark.parametrize("t,family", G.SOFTMAX_CASES)
def test_softmax_bound(t, family):
    G.row_softmax(CPU, t, family)


@pytest.mark.parametrize("kind,affine,family", G.POOL_DW_CASES)
def test_att_pool_dw_bound(kind, affine, family):
    G.row_att_pool_dw(CPU, kind, affine, family)


@pytest.mark.parametrize("act,family", G.KEY_BWD_CASES)
def test_key_backward_bound(act, family):
    G.row_key_backward(CPU, act, family)


@pytest.mark.parametrize("count,act", G.KEY_ACT_CASES)
def test_key_activation_bound(count, act):
    G.row_key_activation(CPU, count, act)


@pytest.mark.parametrize("count,same", G.ADD_CASES)
def test_add_inplace_exact(count, same):
    G.row_add_inplace(CPU, count, same)


@pytest.mark.parametrize("act,use_scale", [(3, True), (0, False), (1, True)])
def test_restatements_are_the_oracles_self_attention(act, use_scale):
    """score -> softmax -> (the oracle's weighted pooling) -> d weights -> softmax backward -> key backward, every piece in float64 from
    tests/attention_ref.py, against O.self_attention_fwd / O.self_attention_bwd on the same data."""
    rs = np.random.RandomState(5 + act)
    b, t, n, dk = 4, 9, 12, 8
    value = np.maximum(rs.randn(b, t, n), 0)
    zk = rs.randn(b * t, dk) * 0.7
    key = A.key_act(zk, act).reshape(b, t, dk)
    q = rs.randn(1, dk) * 0.3
    dout = rs.randn(b, 2 * n)
    pool_ref, pc = O.self_attention_fwd(value, key, q, use_scale)
    dv, dkey, dq_ref = O.self_attention_bwd(value, key, q, pc, dout)
    scale = 1.0 / np.sqrt(dk) if use_scale else 1.0
    score = A.att_score(zk, act, q[0], np.float64(scale))
    w = A.softmax(score.reshape(b, t))
    assert np.allclose(w, pc[0], rtol=1e-6, atol=1e-12)      # (the float32 value of scale: 1 / sqrt(8) rounds at 3e-8)
    dw = A.att_pool_dw(value.reshape(b * t, n), b, t, None, None, 0, None, pool_ref, dout)
    dw_ref = np.einsum("btc,bc->bt", value, dout[:, :n]) + np.einsum("btc,bc->bt", (value - pc[1][:, None, :]) ** 2, dout[:, n:] * 0.5 / pc[2] * (1 - pc[3]))
    assert np.allclose(dw, dw_ref, rtol=1e-9, atol=1e-12)
    ds = A.softmax_backward(pc[0], dw_ref)
    dzk, dq, db = A.key_backward(zk, act, q[0], np.float64(scale), ds.reshape(-1))
    kf = key.reshape(b * t, dk)
    dzk_ref = dkey.reshape(b * t, dk) * ((1 - kf ** 2) if act == 3 else ((zk > 0) if act == 1 else 1.0))
    assert np.allclose(dzk, dzk_ref, rtol=1e-6, atol=1e-12)
    assert np.allclose(dq, dq_ref[0], rtol=1e-6, atol=1e-12)
    assert np.allclose(db, dzk_ref.sum(axis=0), rtol=1e-6, atol=1e-12)
