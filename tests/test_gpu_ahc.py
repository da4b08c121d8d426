"""Agglomerative clustering on a real MI355X: xv_ahc_cluster through ops.ahc_cluster against tests/ahc_ref.py.

The arithmetic is part of the operation (include/xvector_hip.h), so the merge log - the pairs, and the values by their bit patterns - is
asserted EQUAL to the float32 restatement, at every size at which the kernel takes another path: one thread per column (n <= 256), a second
and a third column per thread (257, 600), a repair list longer than one wave.  Agreement with the float64 restatement is asserted on
decision-stable inputs only (ahc_ref.stability >= 8: every decision at least eight fp32 error bounds from every other) - a condition on the
inputs, not a tolerance."""
import numpy as np
import pytest

from tests import ahc_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SIZES = (1, 2, 3, 64, 65, 257, 600)


def _ops():
    import torch
    from tf_kaldi_speaker_amd import ops
    return torch, ops


_DRAWS = {}


def _draw(n):
    """(scores float32 [n, n], the float32 restatement's full run): built once per size, read only."""
    if n not in _DRAWS:
        s, _ = R.clustered_scores(n, n, max(1, min(5, n // 12 + 1)))
        s.setflags(write=False)
        _DRAWS[n] = (s, R.cluster(s, target=1))
    return _DRAWS[n]


def _pack(torch, mats, lds=None, gap=0):
    """The matrices back to back (gap floats between them, pitch lds[i]) in one device buffer filled with NaN where no matrix element
    lies - a read outside a matrix's n columns would poison the result.  -> (buffer, offsets, n, ld)."""
    n = np.asarray([m.shape[0] for m in mats], np.int32)
    ld = n.copy() if lds is None else np.asarray(lds, np.int32)
    offsets = np.concatenate([[0], np.cumsum(n.astype(np.int64) * ld + gap)])[:-1].astype(np.int64) + gap
    host = np.full(int(offsets[-1] + n[-1] * ld[-1] + gap), np.nan, np.float32)
    for m, o, k, l in zip(mats, offsets, n, ld):
        host[o:o + k * l].reshape(k, l)[:, :k] = m
    return torch.from_numpy(host).to(DEV), offsets, n, ld


def _split(out, n):
    """The op's four outputs as per-recording NumPy arrays: [(labels, merges, values)]."""
    labels, merges, values, n_merges = (t.cpu().numpy() for t in out)
    at, mt = np.concatenate([[0], np.cumsum(n)]), np.concatenate([[0], np.cumsum(n - 1)])
    return [(labels[at[i]:at[i + 1]], merges[mt[i]:mt[i] + n_merges[i]], values[mt[i]:mt[i] + n_merges[i]]) for i in range(len(n))]


def _same(got, want):
    labels, merges, values = got
    assert merges.tolist() == want[1].tolist()
    assert values.view(np.int32).tolist() == want[2].view(np.int32).tolist()
    assert labels.tolist() == want[0].tolist()


@pytest.mark.parametrize("n", SIZES)
def test_merge_log_is_bit_equal_to_the_float32_restatement(n):
    torch, ops = _ops()
    s, want = _draw(n)
    buf, off, nn, ld = _pack(torch, [s])
    out = ops.ahc_cluster(buf, off, nn, ld, targets=[1])
    got = _split(out, nn)[0]
    assert len(got[1]) == n - 1
    _same(got, want)
    # the same bits from a second call, and the input is untouched
    again = ops.ahc_cluster(buf, off, nn, ld, targets=[1])
    assert all(torch.equal(a, b) for a, b in zip(out, again))
    assert np.array_equal(buf.cpu().numpy().view(np.int32), _pack(torch, [s])[0].cpu().numpy().view(np.int32))


def test_a_batch_of_mixed_sizes_pitches_beyond_n_and_gaps():
    torch, ops = _ops()
    mats = [_draw(n)[0] for n in (1, 65, 257, 3)]
    buf, off, nn, ld = _pack(torch, mats, lds=[4, 68, 301, 3], gap=5)
    got = _split(ops.ahc_cluster(buf, off, nn, ld, targets=[1, 1, 1, 1]), nn)
    for g, n in zip(got, (1, 65, 257, 3)):
        _same(g, _draw(n)[1])
    # only the upper triangle is read: NaN below the diagonal changes nothing
    low = [m.copy() for m in mats]
    for m in low:
        m[np.tril_indices(m.shape[0], 0)] = np.nan
    buf2, _, _, _ = _pack(torch, low, lds=[4, 68, 301, 3], gap=5)
    for g, n in zip(_split(ops.ahc_cluster(buf2, off, nn, ld, targets=[1, 1, 1, 1]), nn), (1, 65, 257, 3)):
        _same(g, _draw(n)[1])


def test_stop_rules():
    torch, ops = _ops()
    s, full = _draw(65)
    values = full[2]
    mid = 40
    assert values[mid] < values[mid - 1]
    cases = [dict(target=1), dict(target=2), dict(target=65), dict(target=7, threshold=9.0),
             dict(threshold=float(values[mid])),                                             # equal to a merge value: that merge is taken
             dict(threshold=float(np.nextafter(values[mid], np.float32(2)))),               # one ulp above: it is not
             dict(threshold=float(0.5 * (float(values[10]) + float(values[11])))), dict(threshold=2.0), dict(threshold=-2.0)]
    buf, off, nn, ld = _pack(torch, [s] * len(cases))
    for c in cases:      # one call per threshold (a call has one), the targets of all recordings in each
        out = _split(ops.ahc_cluster(buf, off, nn, ld, threshold=c.get("threshold", 0.0), targets=[c.get("target", 0)] * len(cases)), nn)
        want = R.cluster(s, threshold=c.get("threshold", 0.0), target=c.get("target", 0))
        for g in out[:2]:
            _same(g, want)
    # targets differ inside one call
    out = _split(ops.ahc_cluster(buf, off, nn, ld, threshold=float(values[mid]), targets=[0, 1, 2, 65, 7, 0, 0, 0, 0]), nn)
    for g, t in zip(out, [0, 1, 2, 65, 7, 0, 0, 0, 0]):
        _same(g, R.cluster(s, threshold=float(values[mid]), target=t))
    assert len(out[0][1]) == mid + 1 and len(out[3][1]) == 0 and out[3][0].tolist() == list(range(65))


@pytest.mark.parametrize("n", [6, 64, 257, 600])
def test_ties_constant_and_block_constant(n):
    torch, ops = _ops()
    const = np.full((n, n), 0.5, np.float32)
    blocks = np.where(np.subtract.outer(np.arange(n), np.arange(n)) % 3 == 0, 0.75, 0.25).astype(np.float32)      # i = j mod 3: three blocks
    buf, off, nn, ld = _pack(torch, [const, blocks, blocks])
    out = _split(ops.ahc_cluster(buf, off, nn, ld, threshold=0.5, targets=[1, 1, 0]), nn)
    _same(out[0], R.cluster(const, target=1))
    assert out[0][1].tolist() == [[0, k] for k in range(1, n)]
    _same(out[1], R.cluster(blocks, target=1))
    _same(out[2], R.cluster(blocks, threshold=0.5))
    assert out[2][0].tolist() == [i % 3 for i in range(n)]


@pytest.mark.parametrize("n,k", [(3, 2), (17, 2), (65, 3)])
def test_decision_stable_cases_agree_with_float64(n, k):
    torch, ops = _ops()
    draws = [R.clustered_scores(seed, n, k)[0] for seed in range(6)]
    for s in draws:
        assert R.stability(s, target=1).min() >= 8.0      # the condition on the inputs (tests/test_ahc_ref.py pins the figures)
    buf, off, nn, ld = _pack(torch, draws)
    for g, s in zip(_split(ops.ahc_cluster(buf, off, nn, ld, targets=[1] * 6), nn), draws):
        labels, merges, values = R.cluster(s, target=1, dtype=np.float64)
        assert g[1].tolist() == merges.tolist() and g[0].tolist() == labels.tolist()
        # a value's fp32 error is ahc_ref.stability's e = 2^-24 (depth + 1) sum|s| / (size_a size_b): depth <= n - 1 adds, |s| <= 1 (cosines)
        assert np.all(np.abs(g[2].astype(np.float64) - values) <= (n + 1) * 2.0 ** -24 * np.maximum(np.abs(values), 1.0))


def test_refusals():
    torch, ops = _ops()
    from tf_kaldi_speaker_amd import _lib
    from tf_kaldi_speaker_amd._host import _p, _s
    import ctypes as C
    buf = torch.zeros(64, dtype=torch.float32, device=DEV)
    with pytest.raises(ValueError, match="recording 1 has no row"):
        ops.ahc_cluster(buf, [0, 0], [2, 0])
    with pytest.raises(ValueError, match="recording 0 has 2049 rows, the cap is 2048"):
        ops.ahc_cluster(buf, [0], [2049])
    with pytest.raises(ValueError, match="the pitch 3 is below its 4 rows"):
        ops.ahc_cluster(buf, [0], [4], [3])
    with pytest.raises(ValueError, match="target 5 outside 0 .. 4"):
        ops.ahc_cluster(buf, [0], [4], targets=[5])
    with pytest.raises(ValueError, match="target -1 outside"):
        ops.ahc_cluster(buf, [0], [4], targets=[-1])
    with pytest.raises(IndexError, match="a matrix lies outside the 64 floats"):
        ops.ahc_cluster(buf, [0, 49], [4, 4])           # 49 + 3 * 4 + 4 = 65
    with pytest.raises(IndexError, match="a matrix lies outside"):
        ops.ahc_cluster(buf, [-1], [4])
    with pytest.raises(ValueError, match="mat_offsets must be a 1-D integer array of 2"):
        ops.ahc_cluster(buf, [0], [4, 4])
    with pytest.raises(ValueError, match="scores must be a non-empty contiguous 1-D float32 tensor"):
        ops.ahc_cluster(buf.view(8, 8), [0], [4])
    # the library's own refusals, by name
    z = torch.zeros(8, dtype=torch.int32, device=DEV)
    z64 = torch.zeros(8, dtype=torch.int64, device=DEV)
    raw = lambda b, max_n, total, n2, ws_bytes: _lib.call(
        "xv_ahc_cluster", _s(), _p(buf), C.c_int64(64), _p(z64), _p(z), _p(z), _p(z), b, max_n, C.c_int64(total), C.c_int64(n2), C.c_float(0.0),
        _p(z), _p(z), _p(buf), _p(z), _p(buf), C.c_size_t(ws_bytes))
    with pytest.raises(_lib.XvError, match="no recording in the call"):
        raw(0, 4, 4, 16, 256)
    with pytest.raises(_lib.XvError, match="needs at least one row"):
        raw(1, 0, 0, 0, 256)
    with pytest.raises(_lib.XvError, match="2049 rows exceeds the cap of 2048"):
        raw(1, 2049, 2049, 2049 * 2049, 256)
    with pytest.raises(_lib.XvError, match="workspace of 60 bytes, 64 needed"):
        raw(1, 4, 4, 16, 60)
    # and the device still works afterwards
    s, want = _draw(3)
    b3, off, nn, ld = _pack(torch, [s])
    _same(_split(ops.ahc_cluster(b3, off, nn, ld, targets=[1]), nn)[0], want)
