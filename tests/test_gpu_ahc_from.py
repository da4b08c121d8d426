"""The clusterer with a floor and two starts on a real MI355X: xv_ahc_cluster_from through ops.ahc_cluster_from against tests/ahc2_ref.py.

The arithmetic is part of the operation (include/xvector_hip.h), so the merge log - pairs, values by their bit patterns -, the labels and
n_merges are asserted EQUAL to the float32 restatement: at the sizes at which a thread's ownership of columns changes (255, 256, 257, 513),
once at the cap of 2048, from scores and from a seed, with ties, with sizes whose product fp32 does not hold, and with either stop rule
reached first.  Started from scores with the old stop rules the result is ops.ahc_cluster's, bit for bit."""
import ctypes as C

import numpy as np
import pytest

from tests import ahc_ref as R
from tests import ahc2_ref as R2
from tests.test_gpu_ahc import DEV, _ops, _pack, _same, _split

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 3, 255, 256, 257, 513)
NEG_INF = float("-inf")

_SCORES = {}


def _scores(n):
    """Clustered cosine scores [n, n], and the same quantised to quarters (ties at every step); built once per size, read only."""
    if n not in _SCORES:
        s, _ = R.clustered_scores(100 + n, n, max(1, min(5, n // 12 + 1)))
        q = (np.floor(s * 4.0 + 0.5) / 4.0).astype(np.float32)      # (floor: no -0.0, whose sign the restatement's T = U + U^T would drop)
        for m in (s, q):
            m.setflags(write=False)
        _SCORES[n] = (s, q)
    return _SCORES[n]


def _seed(rs, c, top):
    """A symmetric T [c, c] of sums that fit `sizes` (mean scores in -1 .. 1 times the products), sizes in 1 .. top."""
    sizes = rs.randint(1, top + 1, c).astype(np.int64)
    mean = rs.uniform(-1.0, 1.0, (c, c))
    t = np.triu(mean * np.outer(sizes, sizes), 1).astype(np.float32)
    return t + t.T, sizes


def _run_seeded(torch, ops, seeds, floors, threshold=NEG_INF):
    """ops.ahc_cluster_from on seeds [(t, sizes)] -> per-recording (labels, merges, values)."""
    c = np.asarray([t.shape[0] for t, _ in seeds], np.int64)
    flat = torch.from_numpy(np.concatenate([t.ravel() for t, _ in seeds])).to(DEV)
    out = ops.ahc_cluster_from(None, None, c, floors=floors, threshold=threshold, seed=flat, sizes=np.concatenate([s for _, s in seeds]))
    return _split(out, c.astype(np.int32))


@pytest.mark.parametrize("n", SIZES)
def test_from_scores_is_bit_equal_to_the_restatement(n):
    torch, ops = _ops()
    s, q = _scores(n)
    floor = max(1, n // 9)
    buf, off, nn, ld = _pack(torch, [s, q, q], lds=[n + 3, n, n + 1], gap=2)
    got = _split(ops.ahc_cluster_from(buf, off, nn, ld, floors=[floor, 1, floor], threshold=NEG_INF), nn)
    _same(got[0], R2.cluster_from_scores(s, floor))
    _same(got[1], R2.cluster_from_scores(q, 1))
    _same(got[2], R2.cluster_from_scores(q, floor))
    assert [len(g[1]) for g in got] == [n - floor, n - 1, n - floor]
    assert len(np.unique(q)) <= 9      # quarters in -1 .. 1: from n = 5 on the first step already chooses among equal averages


@pytest.mark.parametrize("c", SIZES)
def test_seeded_is_bit_equal_to_the_restatement(c):
    torch, ops = _ops()
    rs = np.random.RandomState(c)
    t, sizes = _seed(rs, c, 40)
    tq = (np.floor(t / 64.0 + 0.5) * 64.0).astype(np.float32)      # coarse sums: equal averages occur
    floor = max(1, c // 11)
    got = _run_seeded(torch, ops, [(t, sizes), (tq, np.ones(c, np.int64)), (t, sizes)], [1, 1, floor])
    _same(got[0], R2.cluster_from(t, sizes, 1))
    _same(got[1], R2.cluster_from(tq, np.ones(c), 1))
    _same(got[2], R2.cluster_from(t, sizes, floor))
    assert len(got[0][1]) == c - 1 and len(got[2][1]) == c - floor


def test_seeded_at_the_cap_of_2048():
    torch, ops = _ops()
    rs = np.random.RandomState(2048)
    t, sizes = _seed(rs, 2048, 16)      # (together at most 32768)
    got = _run_seeded(torch, ops, [(t, sizes)], [1948])[0]
    assert len(got[1]) == 100 and got[1].max() > 1792      # merges that involve the last column a thread owns
    _same(got, R2.cluster_from(t, sizes, 1948))


def test_size_products_above_2_to_the_24_are_rounded_once():
    torch, ops = _ops()
    sizes = np.array([5001, 4999, 5000, 5003, 1, 3, 4997, 7], np.int64)      # 25011 members; 5001 * 4999 = 24999999 is not an fp32 number
    assert float(np.float32(5001 * 4999)) != 5001 * 4999
    rs = np.random.RandomState(9)
    mean = rs.uniform(0.2, 0.9, (8, 8))
    t = np.triu(mean * np.outer(sizes, sizes), 1).astype(np.float32)
    t = t + t.T
    got = _run_seeded(torch, ops, [(t, sizes)], [1])[0]
    want = R2.cluster_from(t, sizes, 1)
    _same(got, want)
    assert len(got[1]) == 7
    # the average of the first pair the restatement divides by the rounded product is what the GPU logged
    a, b = want[1][0]
    assert got[2][0] == t[a, b] / np.float32(int(sizes[a]) * int(sizes[b]))


def test_either_stop_rule_first_and_recordings_of_different_sizes_in_one_call():
    torch, ops = _ops()
    s65, s40, s3 = _scores(65)[0], R.clustered_scores(3, 40, 3)[0], _scores(3)[0]
    values = R.cluster(s65, target=1)[2]
    mid = 40
    assert values[mid] < values[mid - 1]
    between = 0.5 * (float(values[mid - 1]) + float(values[mid]))      # the first `mid` merges are above it
    mats = [s65, s65, s65, s40, s3, s65]
    floors = [50, 5, 65, 7, 1, 1]      # the floor first; the threshold first; floor = n: no merge; ...; ...; threshold equal to a merge value
    buf, off, nn, ld = _pack(torch, mats, lds=[68, 65, 70, 41, 3, 65], gap=3)
    got = _split(ops.ahc_cluster_from(buf, off, nn, ld, floors=floors, threshold=between), nn)
    for g, s, f in zip(got, mats, floors):
        _same(g, R2.cluster_from_scores(s, f, between))
    assert [len(g[1]) for g in got[:3]] == [15, mid, 0] and got[2][0].tolist() == list(range(65))
    exact = _split(ops.ahc_cluster_from(buf, off, nn, ld, floors=floors, threshold=float(values[mid])), nn)
    _same(exact[5], R2.cluster_from_scores(s65, 1, float(values[mid])))
    assert len(exact[5][1]) == mid + 1      # A >= threshold: a merge at the threshold is taken
    # the same bits from a second call
    again = _split(ops.ahc_cluster_from(buf, off, nn, ld, floors=floors, threshold=between), nn)
    for g, h in zip(got, again):
        _same(g, h)


def test_sub_blocks_of_one_matrix_through_offsets():
    torch, ops = _ops()
    s, _ = R.clustered_scores(7, 150, 4)
    buf, off, nn, ld = _pack(torch, [s], lds=[152], gap=4)
    lo = np.asarray([0, 50, 100, 20], np.int64)
    rows = np.asarray([50, 50, 50, 77], np.int64)      # three diagonal blocks of the subset rule, and one that straddles them
    got = _split(ops.ahc_cluster_from(buf, off[0] + lo * 153, rows, np.full(4, 152), floors=[10, 10, 1, 3], threshold=NEG_INF), rows.astype(np.int32))
    for g, a, r, f in zip(got, lo, rows, [10, 10, 1, 3]):
        _same(g, R2.cluster_from_scores(s[a:a + r, a:a + r], f))


@pytest.mark.parametrize("n", [3, 65, 257, 600])
def test_with_the_old_stop_rules_it_is_the_existing_op(n):
    torch, ops = _ops()
    s = R.clustered_scores(n, n, max(1, min(5, n // 12 + 1)))[0]
    values = R.cluster(s, target=1)[2]
    threshold = float(values[len(values) // 2])
    targets = [1, 2, max(1, n // 3), n]
    buf, off, nn, ld = _pack(torch, [s] * 4, lds=[n, n + 1, n, n + 5])
    old = _split(ops.ahc_cluster(buf, off, nn, ld, targets=targets), nn)
    new = _split(ops.ahc_cluster_from(buf, off, nn, ld, floors=targets, threshold=NEG_INF), nn)
    for g, h in zip(new, old):
        _same(g, h)
    old = _split(ops.ahc_cluster(buf, off, nn, ld, threshold=threshold), nn)
    new = _split(ops.ahc_cluster_from(buf, off, nn, ld, floors=[1] * 4, threshold=threshold), nn)
    for g, h in zip(new, old):
        _same(g, h)
    assert n == 3 or 0 < len(new[0][1]) < n - 1      # (the threshold did stop the run midway)


def test_refusals():
    torch, ops = _ops()
    from tf_kaldi_speaker_amd import _lib
    from tf_kaldi_speaker_amd._host import _p, _s
    buf = torch.zeros(64, dtype=torch.float32, device=DEV)
    with pytest.raises(ValueError, match="recording 1 has no row"):
        ops.ahc_cluster_from(buf, [0, 0], [2, 0])
    with pytest.raises(ValueError, match="recording 0 has 2049 rows, the cap is 2048"):
        ops.ahc_cluster_from(buf, [0], [2049])
    with pytest.raises(ValueError, match="the pitch 3 is below its 4 rows"):
        ops.ahc_cluster_from(buf, [0], [4], [3])
    with pytest.raises(ValueError, match="floor 5 outside 1 .. 4"):
        ops.ahc_cluster_from(buf, [0], [4], floors=[5])
    with pytest.raises(ValueError, match="floor 0 outside 1 .. 4"):
        ops.ahc_cluster_from(buf, [0], [4], floors=[0])
    with pytest.raises(IndexError, match="a matrix lies outside the 64 floats"):
        ops.ahc_cluster_from(buf, [0, 49], [4, 4])
    with pytest.raises(ValueError, match="the threshold is NaN"):
        ops.ahc_cluster_from(buf, [0], [4], threshold=float("nan"))
    with pytest.raises(ValueError, match="scores must be a non-empty contiguous 1-D float32 tensor"):
        ops.ahc_cluster_from(buf.view(8, 8), [0], [4])
    with pytest.raises(ValueError, match="sizes belong to a seeded start"):
        ops.ahc_cluster_from(buf, [0], [4], sizes=[1, 1, 1, 1])
    with pytest.raises(ValueError, match="a seeded start reads no scores"):
        ops.ahc_cluster_from(buf, [0], [4], seed=buf, sizes=[1, 1, 1, 1])
    with pytest.raises(ValueError, match="seed must be a contiguous 1-D float32 tensor of at least 81 floats"):
        ops.ahc_cluster_from(None, None, [9], seed=buf, sizes=[1] * 9)
    with pytest.raises(ValueError, match="sizes must be a 1-D integer array of 4"):
        ops.ahc_cluster_from(None, None, [4], seed=buf)
    with pytest.raises(ValueError, match="recording 1: the sizes must be positive and add up to at most 32768"):
        ops.ahc_cluster_from(None, None, [2, 2], seed=buf, sizes=[1, 1, 3, 0])
    with pytest.raises(ValueError, match="recording 0: the sizes must be positive and add up to at most 32768"):
        ops.ahc_cluster_from(None, None, [2, 2], seed=buf, sizes=[30000, 2769, 1, 1])
    with pytest.raises(ValueError, match="recording 0 has 2049 clusters, 1 .. 2048 are taken"):
        ops.ahc_cluster_from(None, None, [2049], seed=buf, sizes=[1] * 2049)
    # the library's own refusals, by name
    z = torch.zeros(8, dtype=torch.int32, device=DEV)
    ones = torch.ones(8, dtype=torch.int32, device=DEV)
    z64 = torch.zeros(8, dtype=torch.int64, device=DEV)
    out = torch.zeros(8, dtype=torch.int32, device=DEV)

    def raw(b, max_n, total, n2, ws_bytes, seeded=0, threshold=0.0, sizes=ones, scores=buf, n=z, floors=ones):
        _lib.call("xv_ahc_cluster_from", _s(), _p(scores), C.c_int64(64), _p(z64), _p(n), _p(n), _p(floors), _p(sizes), seeded, b, max_n, C.c_int64(total),
                  C.c_int64(n2), C.c_float(threshold), _p(out), _p(out), _p(buf), _p(out), _p(buf), C.c_size_t(ws_bytes))

    with pytest.raises(_lib.XvError, match="no recording in the call"):
        raw(0, 4, 4, 16, 256)
    with pytest.raises(_lib.XvError, match="needs at least one row"):
        raw(1, 0, 0, 0, 256)
    with pytest.raises(_lib.XvError, match="2049 rows exceeds the cap of 2048"):
        raw(1, 2049, 2049, 2049 * 2049, 256)
    with pytest.raises(_lib.XvError, match="workspace of 60 bytes, 64 needed"):
        raw(1, 4, 4, 16, 60)
    with pytest.raises(_lib.XvError, match="seeded must be 0 .* or 1 \\(got 2\\)"):
        raw(1, 4, 4, 16, 256, seeded=2)
    with pytest.raises(_lib.XvError, match="the threshold is NaN"):
        raw(1, 4, 4, 16, 256, threshold=float("nan"))
    with pytest.raises(_lib.XvError, match="a seeded start needs the clusters' sizes"):
        raw(1, 4, 4, 16, 256, seeded=1, sizes=None)
    with pytest.raises(_lib.XvError, match="a start from the scores needs scores"):
        raw(1, 4, 4, 16, 256, scores=None)
    # recordings whose device arrays are wrong are skipped with n_merges = -1: a floor of 0, a floor above n, a seeded size of 0, sizes
    # that add up to more than 32768 - and the device still works afterwards
    four = torch.full((8,), 4, dtype=torch.int32, device=DEV)
    for kw in (dict(floors=z), dict(floors=torch.full((8,), 5, dtype=torch.int32, device=DEV)), dict(seeded=1, sizes=z),
               dict(seeded=1, sizes=torch.full((8,), 9000, dtype=torch.int32, device=DEV))):
        out.zero_()
        raw(1, 4, 4, 16, 256, n=four, **kw)
        assert int(out[0]) == -1, kw
    s, _ = _scores(3)
    b3, off, nn, ld = _pack(torch, [s])
    _same(_split(ops.ahc_cluster_from(b3, off, nn, ld), nn)[0], R2.cluster_from_scores(s))
