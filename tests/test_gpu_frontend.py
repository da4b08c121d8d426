"""xv_frontend on a real MI355X: sliding-window CMN and voiced-frame selection on a padded batch against the fp64 restatement
(tests/frontend_ref.py).  Inputs are MFCC-like (randn * 20 + 50, column 0 shifted by -120); with A the utterance's max |x| the bound is
|got - ref| <= 2^-23 |ref| + 2^-32 A: ONE fp32 rounding of a mean accumulated in double (an fp32 accumulation of any kind - prefix sums,
running add / remove, pairwise - is 5e-7 .. 7e-6 of A at 4000 frames and does not pass).  Selection alone (window 0) is bit-exact."""
import numpy as np
import pytest

from tests import frontend_ref as R

pytestmark = pytest.mark.gpu

LENS = [1, 149, 150, 151, 299, 300, 301, 450, 1000, 4000, 450, 700]       # the window's edge cases (w = 300) + an unvoiced and a random piece
DIMS = [1, 30, 40, 128]


def _masks(lens, seed=11):
    """One voicing mask per piece: all voiced, only the first frame, only the last, alternating, runs that cross frame 64 and frame 256
    (wave and workgroup seams of the scan), nothing voiced, ~70 % random."""
    rs = np.random.RandomState(seed)
    out = []
    for i, n in enumerate(lens):
        m = np.zeros(n, np.uint8)
        if n == 4000:
            for a, b in ((60, 70), (250, 262), (500, 900), (1020, 1030), (3999, 4000)):
                m[a:b] = 1
            m[2000:3000] = rs.rand(1000) < 0.3
        elif n == 1000:
            m[::2] = 1                                     # alternating
        elif n == 301:
            m[0] = 1                                       # only the first frame
        elif n == 300:
            m[-1] = 1                                      # only the last frame
        elif n == 450 and i == 7:
            m[50:70] = 7                                   # any non-zero byte is voiced; the run crosses frame 64
            m[200:300] = 1                                 # ... and this one frame 256
        elif n == 450:
            pass                                           # nothing voiced
        elif n == 700:
            m[:] = rs.rand(n) < 0.7
        else:
            m[:] = 1                                       # all voiced
        out.append(m)
    return out


def _pack_masks(masks):
    """Back to back behind one stray byte, so the offsets have no alignment at all."""
    offs, parts, at = [], [np.array([9], np.uint8)], 1
    for m in masks:
        offs.append(at)
        parts.append(m)
        at += len(m)
    assert any(o % 2 for o in offs) and any(o % 4 == 2 for o in offs)
    return np.concatenate(parts), np.asarray(offs, np.int64)


@pytest.fixture(scope="module")
def data():
    """Raw utterances at the widest dimension (narrower cases take its leading columns) and their fp64 CMN; computed once, read only."""
    rs = np.random.RandomState(21)
    utts = [R.raw_features(rs, n, max(DIMS)) for n in LENS]
    for u in utts:
        u.setflags(write=False)
    cmn = {}

    def ref(i, d, w):
        if (i, d, w) not in cmn:
            y = R.sliding_cmn(utts[i][:, :d], w)
            y.setflags(write=False)
            cmn[(i, d, w)] = y
        return cmn[(i, d, w)]
    return utts, ref


def _run(utts, d, w, masks=None, first=None, count=None, t_out=None, lens=None):
    import torch
    from tf_kaldi_speaker_amd import ops
    dev = torch.device("cuda:0")
    lens = [len(u) for u in utts] if lens is None else lens
    t_in = max(lens)                                      # the longest piece has no padding at all
    x = np.full((len(utts), t_in, d), 1e4, np.float32)    # rows behind an utterance are NOT zero: they must not reach any mean
    for i, u in enumerate(utts):
        x[i, :lens[i]] = u[:lens[i], :d]
    xd = torch.from_numpy(x).to(dev)
    rows = torch.tensor(lens, dtype=torch.int32, device=dev)
    md = od = None
    if masks is not None:
        buf, offs = _pack_masks(masks)
        md, od = torch.from_numpy(buf).to(dev), torch.from_numpy(offs).to(dev)
    fd = None if first is None else torch.tensor(first, dtype=torch.int32, device=dev)
    cd = None if count is None else torch.tensor(count, dtype=torch.int32, device=dev)
    out, rows_out = ops.frontend(xd, rows, w, md, od, fd, cd, t_out)
    out2, rows_out2 = ops.frontend(xd, rows, w, md, od, fd, cd, t_out)
    torch.cuda.synchronize()
    got, got2 = out.cpu().numpy(), out2.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), got2.view(np.uint32)), "two calls on the same input differ"
    assert np.array_equal(rows_out.cpu().numpy(), rows_out2.cpu().numpy())
    return got, rows_out.cpu().numpy()


def _check(got, rows_out, utts, ref, d, w, masks, first, count, exact=False):
    worst = 0.0
    for i, u in enumerate(utts):
        y = ref(i, d, w)
        if masks is not None:
            y = y[np.flatnonzero(masks[i])]
        y = y[(first[i] if first is not None else 0):]
        if count is not None:
            y = y[:count[i]]
        assert rows_out[i] == len(y), (i, rows_out[i], len(y))          # the host's count
        g = got[i, :len(y)]
        assert not got[i, len(y):].any(), "piece %d: padding rows are not exactly zero" % i
        if exact:
            assert np.array_equal(g.view(np.uint32), y.astype(np.float32).view(np.uint32)), i
            continue
        a = float(np.abs(u[:, :d]).max())
        excess = np.abs(g.astype(np.float64) - y) - (2.0 ** -23 * np.abs(y) + 2.0 ** -32 * a)
        if len(y):
            worst = max(worst, float((np.abs(g.astype(np.float64) - y) / a).max()))
            assert excess.max() <= 0, (i, len(u), float(excess.max()), a)
    print("d=%d w=%d: worst |got - ref| / A = %.3g" % (d, w, worst))


@pytest.mark.parametrize("d", DIMS)
def test_cmn_then_selection(data, d):
    utts, ref = data
    masks = _masks(LENS)
    t_out = max(int(np.count_nonzero(m)) for m in masks)
    got, rows_out = _run(utts, d, 300, masks, t_out=t_out)
    assert got.shape == (len(LENS), t_out, d)
    _check(got, rows_out, utts, ref, d, 300, masks, None, None)


@pytest.mark.parametrize("d", [30, 128])
def test_selection_only_is_bit_exact(data, d):
    utts, ref = data
    masks = _masks(LENS)
    t_out = max(int(np.count_nonzero(m)) for m in masks) + 5
    got, rows_out = _run(utts, d, 0, masks, t_out=t_out)
    _check(got, rows_out, utts, ref, d, 0, masks, None, None, exact=True)


@pytest.mark.parametrize("d", [1, 30, 128])
def test_cmn_only_without_masks(data, d):
    utts, ref = data
    got, rows_out = _run(utts, d, 300)
    assert got.shape == (len(LENS), max(LENS), d)
    _check(got, rows_out, utts, ref, d, 300, None, None, None)


@pytest.mark.parametrize("with_masks", [True, False], ids=["masks", "no-masks"])
def test_chunk_pieces_first_and_count(data, with_masks):
    """first > 0 with count smaller than what remains (the chunks of a long utterance), count larger than what remains, first beyond the
    last kept frame."""
    utts, ref = data
    masks = _masks(LENS) if with_masks else None
    kept = [int(np.count_nonzero(m)) for m in masks] if with_masks else list(LENS)
    first = [0, 10, 149, 75, 3, 0, 0, 60, 150, kept[9] // 2, 0, 333]
    count = [1, 50, 5, 76, 400, 1, 1, 30, 300, 250, 10, 200]
    first[5], first[6] = (0, 0) if with_masks else (299, 1)
    first[10] = 0 if with_masks else 500                  # beyond the last frame of a 450-frame piece: nothing is kept
    got, rows_out = _run(utts, 30, 300, masks, first, count, t_out=max(count))
    assert any(f > 0 and f + c < k for f, c, k in zip(first, count, kept)) and any(f + c > k for f, c, k in zip(first, count, kept))
    _check(got, rows_out, utts, ref, 30, 300, masks, first, count)


@pytest.mark.parametrize("w", [7, 8])
def test_short_windows_odd_and_even(w):
    """Windows of 7 and 8 frames (the integer division in t - w / 2) on utterances around the window length, alternating masks."""
    lens = [1, 3, 4, 7, 8, 9, 20]
    rs = np.random.RandomState(31 + w)
    utts = [R.raw_features(rs, n, 30) for n in lens]
    masks = []
    for n in lens:
        m = np.zeros(n, np.uint8)
        m[(n % 2)::2] = 1
        m[0] = 1
        masks.append(m)
    ref = lambda i, d, ww: R.sliding_cmn_loop(utts[i][:, :d], ww)      # noqa: E731 - the literal loop: these are tiny
    for mk in (masks, None):
        got, rows_out = _run(utts, 30, w, mk)
        _check(got, rows_out, utts, ref, 30, w, mk, None, None)


def test_rows_in_shorter_than_the_buffer_and_bad_arguments(data):
    """rows_in below t_in for EVERY piece (windows end at the utterance, not at the buffer), and the arguments the entry point refuses."""
    import torch
    from tf_kaldi_speaker_amd import ops, _lib
    utts, ref = data
    sub = [utts[i] for i in (1, 4, 7)]
    x = np.full((3, 500, 30), -3e3, np.float32)
    for i, u in enumerate(sub):
        x[i, :len(u)] = u[:, :30]
    dev = torch.device("cuda:0")
    rows = torch.tensor([len(u) for u in sub], dtype=torch.int32, device=dev)
    out, rows_out = ops.frontend(torch.from_numpy(x).to(dev), rows, 300)
    _check(out.cpu().numpy(), rows_out.cpu().numpy(), sub, lambda i, d, w: ref((1, 4, 7)[i], d, w), 30, 300, None, None, None)
    with pytest.raises(_lib.XvError, match="at most 128"):
        ops.frontend(torch.zeros((1, 4, 129), device=dev), rows[:1], 0)
    with pytest.raises(_lib.XvError, match="CMN window"):
        ops.frontend(torch.zeros((1, 4, 30), device=dev), rows[:1], -1)
    # a workspace one byte short of b * t_out * 4 is refused (nothing is launched)
    xs, o = torch.zeros((1, 4, 30), device=dev), torch.zeros((1, 4, 30), device=dev)
    m, mo = torch.ones(4, dtype=torch.uint8, device=dev), torch.zeros(1, dtype=torch.int64, device=dev)
    ro, ws = torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(4, dtype=torch.int32, device=dev)
    p = lambda t: t.data_ptr()      # noqa: E731
    rc = _lib.load().xv_frontend(None, p(xs), p(rows), 1, 4, 30, 0, p(m), 4, p(mo), None, None, 4, p(o), p(ro), p(ws), 15)
    assert rc != 0 and b"workspace" in _lib.load().xv_last_error()
