"""xv_cm_encode (ops.cm_encode) on a real MI355X against the unchanged host writer dataset.kaldi_io.write_compressed_mat and the host
decoder _decode_cm - never the kernel against itself.  The only tolerance is byte equality, in both header forms.  Every compared matrix
has four distinct fp32 header points in every column (asserted on the host with _col_percentiles, no case is left out): where two points
coincide the host writer casts NaN to uint8, which is outside the byte contract (include/xvector_hip.h) - that case has its own test.
Padding rows are filled with 1e30 everywhere: a kernel that reads one fails on the global header."""
import io

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROWS = [1, 2, 3, 4, 5, 7, 8, 63, 64, 65, 255, 256, 257, 1025, 4099]      # the small-matrix branch, rows / 4 arithmetic, > 1 histogram chunk and code tile
DIMS = [1, 3, 30, 31, 128]
HEADERS = ["quartiles", "uniform"]
DISTRIBUTIONS = ["normal", "wide_with_constant_column", "halves", "constant", "column_at_maximum"]
PAD = np.float32(1e30)


def _matrices(dist, d, seed):
    """The matrices of one distribution at d columns, one per row count (constant: three values x a few row counts)."""
    rs = np.random.RandomState(seed)
    out = []
    if dist == "constant":
        for value in (0.0, -3.25, 7.0):
            out += [np.full((rows, d), value, np.float32) for rows in (1, 4, 6, 257)]
        return out
    for rows in ROWS:
        if dist == "normal":
            m = rs.randn(rows, d).astype(np.float32)
        elif dist == "wide_with_constant_column":      # the log-energy floor beside wide cepstra
            m = (rs.randn(rows, d) * 30.0).astype(np.float32)
            m[:, 0] = np.float32(-15.9424)
        elif dist == "halves":                         # the ranks cut through runs of equal values
            m = (np.round(rs.randn(rows, d) * 2.0) / 2.0).astype(np.float32)
        else:                                          # rows 1 .. 4 with a column at the matrix maximum: 65535 + 1 wraps to 0 in uint16
            if rows > 4:
                continue
            m = rs.randn(rows, d).astype(np.float32)
            m[:, d - 1] = m.max()
        out.append(m)
    return out


def _host_image(m, header):
    from tf_kaldi_speaker_amd.dataset import kaldi_io
    buf = io.BytesIO()
    kaldi_io.write_compressed_mat(buf, m, key="", header=header)
    image = buf.getvalue()
    assert image[:5] == b"\0BCM "
    return image[5:]


def _points(image):
    """[cols, 4] float32 header points of an image, as every reader computes them."""
    from tf_kaldi_speaker_amd.dataset import kaldi_io
    gmin, grange, rows, cols = np.frombuffer(image[:16], dtype=kaldi_io._GLOBAL_HDR, count=1)[0]
    return kaldi_io._col_percentiles(np.frombuffer(image[16:16 + 8 * cols], dtype=kaldi_io._COL_HDR, count=cols), gmin, grange)


def _batch(mats, t=None, device="cuda"):
    import torch
    t = max(len(m) for m in mats) + 3 if t is None else t
    x = np.full((len(mats), t, mats[0].shape[1]), PAD, np.float32)
    for i, m in enumerate(mats):
        x[i, :len(m)] = m
    return torch.from_numpy(x).to(device), np.asarray([len(m) for m in mats], np.int64)


def _encode(mats, header, t=None):
    """(the images the kernel wrote, the whole buffer, its offsets)."""
    import torch
    from tf_kaldi_speaker_amd import ops
    x, rows = _batch(mats, t)
    out, offsets = ops.cm_encode(x, rows, header=header)
    torch.cuda.synchronize()
    sizes = ops.cm_image_bytes(rows, mats[0].shape[1])
    assert out.dtype == torch.uint8 and out.numel() == int(sizes.sum()) and np.array_equal(offsets, np.cumsum(sizes) - sizes)
    raw = out.cpu().numpy().tobytes()
    return [raw[o:o + n] for o, n in zip(offsets, sizes)], out, offsets


def _assert_equal(got, want, what):
    if got != want:
        first = next(i for i, (a, b) in enumerate(zip(got, want)) if a != b)
        raise AssertionError("%s: %d of %d bytes differ, the first at byte %d (got %d, the host writer %d)"
                             % (what, sum(a != b for a, b in zip(got, want)), len(want), first, got[first], want[first]))


@pytest.mark.parametrize("dist", DISTRIBUTIONS)
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("header", HEADERS)
def test_bytes_equal_the_host_writer(header, d, dist):
    mats = _matrices(dist, d, seed=1000 * DIMS.index(d) + DISTRIBUTIONS.index(dist))
    want = [_host_image(m, header) for m in mats]
    for m, image in zip(mats, want):      # inside the byte contract: asserted, not skipped
        assert (np.diff(_points(image), axis=1) > 0).all(), "%s %s d=%d rows=%d: two header points coincide" % (header, dist, d, len(m))
    got, _, _ = _encode(mats, header)
    for m, g, w in zip(mats, got, want):
        _assert_equal(g, w, "%s %s d=%d rows=%d value[0,0]=%r" % (header, dist, d, len(m), float(m[0, 0])))


def _ragged(b, d, seed):
    rs = np.random.RandomState(seed)
    lens = [int(n) for n in rs.choice([1, 2, 3, 4, 5, 6, 9, 33, 64, 65, 100, 129, 300, 511], size=b)]
    return [(rs.randn(n, d) * rs.choice([0.5, 3.0, 40.0])).astype(np.float32) for n in lens]


@pytest.mark.parametrize("header", HEADERS)
@pytest.mark.parametrize("b", [1, 37])
def test_ragged_batch_in_one_call(b, header):
    """Mixed row counts in one call, t beyond every rows[i], images back to back: d = 31 makes odd and 2-mod-4 offsets."""
    mats = _ragged(b, 31, seed=5 + b)
    got, _, offsets = _encode(mats, header, t=600)
    if b > 1:
        assert any(o % 2 for o in offsets) and any(o % 4 == 2 for o in offsets)
    for i, m in enumerate(mats):
        want = _host_image(m, header)
        assert (np.diff(_points(want), axis=1) > 0).all()
        _assert_equal(got[i], want, "%s piece %d of %d, rows=%d" % (header, i, b, len(m)))


@pytest.mark.parametrize("header", HEADERS)
def test_round_trip_through_the_device_decoder(header):
    """ops.cm_decode_ragged on the encoder's buffer == the host decoder on the host writer's bytes, bit for bit."""
    import torch
    from tf_kaldi_speaker_amd import ops
    from tf_kaldi_speaker_amd.dataset import kaldi_io
    mats = _ragged(11, 30, seed=77)
    _, buf, offsets = _encode(mats, header, t=600)
    rows = [len(m) for m in mats]
    y = ops.cm_decode_ragged(buf, offsets, rows, 520, 30)
    torch.cuda.synchronize()
    y = y.cpu().numpy()
    for i, m in enumerate(mats):
        want = kaldi_io.read_mat(io.BytesIO(b"\0BCM " + _host_image(m, header)))
        assert want.shape == m.shape and np.array_equal(y[i, :rows[i]].view(np.uint32), want.view(np.uint32)), i
        assert not y[i, rows[i]:].any()


@pytest.mark.parametrize("header", HEADERS)
def test_same_bytes_on_every_call_and_in_every_position(header):
    mats = _ragged(5, 30, seed=3)
    first, _, _ = _encode(mats, header, t=600)
    again, _, _ = _encode(mats, header, t=600)
    assert first == again
    alone, _, _ = _encode([mats[2]], header, t=len(mats[2]))      # alone, with no padding row at all
    assert alone[0] == first[2] == _host_image(mats[2], header)


@pytest.mark.parametrize("header", HEADERS)
def test_degenerate_column_keeps_header_and_code_ranges(header):
    """rows = 2, values 5 +- 1e-3, column 0 constant at 5 (the evenly spaced points of a column with some range stay apart): the header's
    steps fall below the fp32 spacing at 5, so points coincide and the host writer's codes are platform-defined.  The header bytes still
    equal the host's, every code lies inside the range of its branch, the call succeeds."""
    rs = np.random.RandomState(9)
    m = (5.0 + 1e-3 * rs.uniform(-1.0, 1.0, size=(2, 3))).astype(np.float32)
    m[:, 0] = 5.0
    with np.errstate(invalid="ignore"):
        want = _host_image(m, header)
    pts = _points(want)
    assert (np.diff(pts, axis=1) == 0).any(), "the case is meant to have coinciding header points"
    (got,), _, _ = _encode([m], header)
    assert got[:16 + 8 * 3] == want[:16 + 8 * 3]
    codes = np.frombuffer(got[16 + 8 * 3:], np.uint8).reshape(3, 2)
    for c in range(3):
        for r in range(2):
            lo, hi = (0, 64) if m[r, c] < pts[c, 1] else (64, 192) if m[r, c] < pts[c, 2] else (192, 255)
            assert lo <= codes[c, r] <= hi, (c, r, int(codes[c, r]), lo, hi)


def test_refusals_by_name():
    import torch
    from tf_kaldi_speaker_amd import ops
    x = torch.zeros((2, 8, 30), dtype=torch.float32, device="cuda")
    with pytest.raises(IndexError, match="cm_encode: rows holds a value outside 1 .. 8"):
        ops.cm_encode(x, [3, 0])
    with pytest.raises(IndexError, match="cm_encode: rows holds a value outside 1 .. 8"):
        ops.cm_encode(x, [9, 3])
    with pytest.raises(ValueError, match="cm_encode: rows must be a non-empty 1-D integer array of 2"):
        ops.cm_encode(x, [3])
    with pytest.raises(ValueError, match="cm_encode: d must lie in 1 .. 128 \\(got 129\\)"):
        ops.cm_encode(torch.zeros((1, 4, 129), dtype=torch.float32, device="cuda"), [4])
    with pytest.raises(ValueError, match="cm_encode: header must be 'quartiles' or 'uniform' \\(got 'deciles'\\)"):
        ops.cm_encode(x, [3, 3], header="deciles")
    with pytest.raises(ValueError, match="cm_encode: x must be a contiguous float32"):
        ops.cm_encode(x.double(), [3, 3])
