"""Cluster sums on a real MI355X: xv_ahc_cluster_sums through ops.ahc_cluster_sums against tests/ahc2_ref.py.

The order of every sum is part of the operation (include/xvector_hip.h), so the seed T and the sizes are asserted EQUAL to the
restatement, bit for bit: around the 64 rows a wave of the rows kernel takes (63, 64, 65), with more than one workgroup per recording
(300), with one cluster, with singletons only and with interleaved members, on a pitch above n.  The lower triangle and the diagonal
hold NaN: a read of either would poison the result."""
import ctypes as C

import numpy as np
import pytest

from tests import ahc2_ref as R2
from tests.test_gpu_ahc import DEV, _ops, _pack

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 300)

_CASES = {}


def _partitions(n):
    """{name: labels numbered by smallest member}: everything in one cluster, singletons, interleaved members in 3 and in 7 clusters
    (cluster sizes on either side of the kernels' unrolling), contiguous runs of uneven length."""
    rs = np.random.RandomState(n)
    cuts = np.sort(rs.choice(np.arange(1, n), size=min(n - 1, 5), replace=False)) if n > 1 else np.zeros(0, np.int64)
    return {"one": np.zeros(n, np.int64), "singletons": np.arange(n), "mod3": np.arange(n) % min(3, n), "mod7": np.arange(n) % min(7, n),
            "runs": np.searchsorted(cuts, np.arange(n), side="right")}


def _case(n):
    """(scores float32 [n, n] with NaN on and below the diagonal, {name: (labels, restated T, restated sizes)}); built once, read only."""
    if n not in _CASES:
        s = np.random.RandomState(1000 + n).randn(n, n).astype(np.float32)
        s[np.tril_indices(n, 0)] = np.nan
        s.setflags(write=False)
        _CASES[n] = (s, {k: (lab,) + R2.cluster_sums(s, R2.member_lists(lab)) for k, lab in _partitions(n).items()})
    return _CASES[n]


def _sums(torch, ops, mats, labels, lds=None, gap=0):
    """ops.ahc_cluster_sums on the matrices with one labelling each -> per recording (T [c, c], sizes [c])."""
    buf, off, nn, ld = _pack(torch, mats, lds=lds, gap=gap)
    members, starts, c = ops.ahc_member_lists(np.concatenate(labels), nn)
    seed, sizes = ops.ahc_cluster_sums(buf, off, nn, ld, members, starts, c)
    seed, sizes = seed.cpu().numpy(), sizes.cpu().numpy()
    assert seed.size == int((c * c).sum()) and sizes.size == int(c.sum())
    at, ct = np.concatenate([[0], np.cumsum(c * c)]), np.concatenate([[0], np.cumsum(c)])
    return [(seed[at[i]:at[i + 1]].reshape(c[i], c[i]), sizes[ct[i]:ct[i + 1]]) for i in range(len(mats))]


def _equal(got, want):
    assert got[1].tolist() == want[1].tolist()
    assert got[0].shape == want[0].shape and np.array_equal(got[0].view(np.int32), want[0].view(np.int32))
    assert np.array_equal(got[0].view(np.int32), got[0].T.view(np.int32)) and not np.isnan(got[0]).any()      # symmetric bit for bit
    assert (np.diag(got[0]).view(np.int32) == 0).all()


@pytest.mark.parametrize("n", SIZES)
def test_seed_and_sizes_are_bit_equal_to_the_restatement(n):
    torch, ops = _ops()
    s, cases = _case(n)
    names = list(cases)
    # every labelling of this size in one call, on the matrix's own pitch and on a larger one
    for lds in (None, [n + 1 + k for k in range(len(names))]):
        got = _sums(torch, ops, [s] * len(names), [cases[k][0] for k in names], lds=lds, gap=3)
        for g, k in zip(got, names):
            _equal(g, cases[k][1:])
    assert cases["one"][1].tolist() == [[0.0]] and cases["one"][2].tolist() == [n]
    assert cases["singletons"][2].tolist() == [1] * n


def test_two_recordings_of_different_sizes_in_one_call_and_the_same_bits_twice():
    torch, ops = _ops()
    (s300, c300), (s65, c65), (s1, c1) = _case(300), _case(65), _case(1)
    mats, labels = [s300, s65, s1, s300], [c300["mod7"][0], c65["runs"][0], c1["one"][0], c300["singletons"][0]]
    got = _sums(torch, ops, mats, labels, lds=[304, 65, 1, 300], gap=1)
    for g, want in zip(got, (c300["mod7"], c65["runs"], c1["one"], c300["singletons"])):
        _equal(g, want[1:])
    again = _sums(torch, ops, mats, labels, lds=[304, 65, 1, 300], gap=1)
    for g, h in zip(got, again):
        _equal(g, h)


def test_the_seed_feeds_the_seeded_clusterer():
    """What the two ops hand each other: the seed of a labelling, clustered on from there, against the restatement of both."""
    torch, ops = _ops()
    s = np.abs(_case(65)[0])
    lab = _partitions(65)["mod7"]
    buf, off, nn, ld = _pack(torch, [s])
    members, starts, c = ops.ahc_member_lists(lab, nn)
    seed, sizes = ops.ahc_cluster_sums(buf, off, nn, ld, members, starts, c)
    labels, merges, values, n_merges = ops.ahc_cluster_from(None, None, c, floors=[2], seed=seed, sizes=sizes.cpu().numpy())
    t, want_sizes = R2.cluster_sums(s, R2.member_lists(lab))
    want = R2.cluster_from(t, want_sizes, 2)
    assert int(n_merges[0]) == 5 and merges.cpu().numpy()[:5].tolist() == want[1].tolist() and labels.cpu().numpy().tolist() == want[0].tolist()
    assert values.cpu().numpy()[:5].view(np.int32).tolist() == want[2].view(np.int32).tolist()


def test_refusals():
    torch, ops = _ops()
    from tf_kaldi_speaker_amd import _lib
    from tf_kaldi_speaker_amd._host import _p, _s
    buf = torch.zeros(64, dtype=torch.float32, device=DEV)
    ok = dict(members=[0, 2, 1, 3], starts=[0, 2, 4], c=[2])
    call = lambda **kw: ops.ahc_cluster_sums(buf, kw.get("off", [0]), kw.get("n", [4]), kw.get("ld", None), kw.get("members", ok["members"]),
                                            kw.get("starts", ok["starts"]), kw.get("c", ok["c"]))
    with pytest.raises(ValueError, match="recording 0 has 32769 rows, the cap is 32768"):
        call(n=[32769])
    with pytest.raises(ValueError, match="the pitch 3 is below its 4 rows"):
        call(ld=[3])
    with pytest.raises(IndexError, match="a matrix lies outside the 64 floats"):
        call(off=[49])
    with pytest.raises(ValueError, match="recording 0 has 5 clusters, 1 .. 4 are taken"):
        call(c=[5])
    with pytest.raises(ValueError, match="recording 0 has 0 clusters"):
        call(c=[0])
    with pytest.raises(ValueError, match="starts must be a 1-D integer array of 3"):
        call(starts=[0, 4])
    with pytest.raises(ValueError, match="starts must ascend from 0 to its 4 rows"):
        call(starts=[0, 2, 3])
    with pytest.raises(ValueError, match="starts must ascend from 0 to its 4 rows"):
        call(starts=[0, 0, 4])
    with pytest.raises(ValueError, match="members must hold every row once"):
        call(members=[0, 2, 1, 1])
    with pytest.raises(ValueError, match="members must hold every row once"):
        call(members=[2, 0, 1, 3])      # a cluster's members ascending
    with pytest.raises(ValueError, match="members must hold every row once"):
        call(members=[1, 3, 0, 2])      # clusters ascending by smallest member
    with pytest.raises(ValueError, match="labels must be 0, 1, ... in the order of the clusters' smallest members"):
        ops.ahc_member_lists([1, 0, 1], [3])
    # the library's own refusals, by name
    z = torch.zeros(8, dtype=torch.int32, device=DEV)
    z64 = torch.zeros(8, dtype=torch.int64, device=DEV)
    out = torch.zeros(8, dtype=torch.int32, device=DEV)
    ws = torch.zeros(64, dtype=torch.float64, device=DEV)

    def raw(b=1, max_n=4, max_c=2, total_n=4, total_c=2, sum_c2=4, sum_nc=8, ws_bytes=512, n=z, c=z, members=z, starts=z):
        _lib.call("xv_ahc_cluster_sums", _s(), _p(buf), C.c_int64(64), _p(z64), _p(n), _p(n), _p(c), _p(members), _p(starts), b, max_n, max_c,
                  C.c_int64(total_n), C.c_int64(total_c), C.c_int64(sum_c2), C.c_int64(sum_nc), _p(buf), _p(out), _p(out[4:]), _p(ws), C.c_size_t(ws_bytes))

    with pytest.raises(_lib.XvError, match="1 .. 65535 recordings in a call"):
        raw(b=0)
    with pytest.raises(_lib.XvError, match="a recording of 32769 rows exceeds the cap of 32768"):
        raw(max_n=32769, total_n=32769, sum_nc=65538)
    with pytest.raises(_lib.XvError, match="2049 clusters exceed the cap of 2048"):
        raw(max_n=4096, max_c=2049, total_n=4096, total_c=2049, sum_c2=2049 * 2049, sum_nc=4096 * 2049)
    with pytest.raises(_lib.XvError, match="5 clusters exceed the cap of 2048 \\(or the 4 rows\\)"):
        raw(max_c=5, total_c=5, sum_c2=25, sum_nc=20)
    with pytest.raises(_lib.XvError, match="do not fit b recordings of at most 4 rows and 2 clusters"):
        raw(sum_nc=9)
    with pytest.raises(_lib.XvError, match="workspace of 88 bytes, 96 needed"):
        raw(ws_bytes=88)
    # device arrays that are wrong: the recording is skipped with status -1 (no rows; starts that do not reach n; a member outside the rows)
    four, two = torch.full((8,), 4, dtype=torch.int32, device=DEV), torch.full((8,), 2, dtype=torch.int32, device=DEV)
    good_starts = torch.tensor([0, 2, 4], dtype=torch.int32, device=DEV)
    good_members = torch.tensor([0, 2, 1, 3], dtype=torch.int32, device=DEV)
    for kw in (dict(n=z, c=two, members=good_members, starts=good_starts), dict(n=four, c=two, members=good_members, starts=z),
               dict(n=four, c=two, members=torch.tensor([0, 2, 1, 4], dtype=torch.int32, device=DEV), starts=good_starts)):
        out.zero_()
        raw(**kw)
        assert int(out[4]) == -1, kw
    out.zero_()
    raw(n=four, c=two, members=good_members, starts=good_starts)
    assert int(out[4]) == 0 and out[:2].tolist() == [2, 2]
