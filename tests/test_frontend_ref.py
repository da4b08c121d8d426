"""The front end's reference (tests/frontend_ref.py) against a literal per-frame loop, and the host rules of the extraction driver with
--cmn-window / --vad (which utterances are skipped, chunking in post-selection frames) - no GPU."""
import io
import os

import numpy as np
import pytest

from tests import frontend_ref as R
from tf_kaldi_speaker_amd.dataset import kaldi_io
from tf_kaldi_speaker_amd.misc import utils

CASES = [(300, n) for n in (1, 149, 150, 151, 299, 300, 301, 450, 1000, 4000)] + [(w, n) for w in (7, 8) for n in (1, 3, 4, 7, 8, 9, 20)]


@pytest.mark.parametrize("w,n", CASES)
def test_restatement_equals_the_per_frame_loop(w, n):
    rs = np.random.RandomState(1000 * w + n)
    x = R.raw_features(rs, n, 5)
    got, ref = R.sliding_cmn(x, w), R.sliding_cmn_loop(x, w)
    # two float64 evaluations of the same mean: a direct sum of up to w terms of size A carries at most w * 2^-53 * A
    a = float(np.abs(x).max())
    assert np.abs(got - ref).max() <= w * 2.0 ** -53 * a
    s, e = R.window_bounds(n, w)
    assert np.all((0 <= s) & (s < e) & (e <= n)) and np.all(e - s == min(w, n))
    t = np.arange(n)
    assert np.all((s <= t) & (t < e))                     # a frame is always inside its own window
    if n > w:                                              # away from the ends the window is centred: w // 2 frames in front
        mid = (t >= w // 2) & (t + (w - w // 2) <= n)
        assert np.all(s[mid] == t[mid] - w // 2)


def test_window_off_and_selection_order():
    rs = np.random.RandomState(2)
    x = R.raw_features(rs, 40, 3)
    assert np.array_equal(R.frontend(x, 0), x.astype(np.float64))
    mask = (rs.rand(40) < 0.5).astype(np.uint8)
    y = R.sliding_cmn(x, 8)
    sel = np.flatnonzero(mask)
    assert np.array_equal(R.frontend(x, 8, mask), y[sel])              # CMN sees the raw utterance, selection comes second
    assert np.array_equal(R.frontend(x, 8, mask, first=3, count=5), y[sel[3:8]])


def test_select_voiced_skip_rules_and_lengths():
    rs = np.random.RandomState(3)
    feat = rs.randn(50, 4).astype(np.float32)
    rows, skip = utils.select_voiced("u0", feat, None)
    assert rows is None and skip == "[INFO] Key u0 has no VAD entry, skip."
    rows, skip = utils.select_voiced("u1", feat, np.ones(49, np.float32))
    assert rows is None and skip == "[INFO] Key u1 has 50 frames but 49 VAD decisions, skip."
    rows, skip = utils.select_voiced("u2", feat, np.zeros(50, np.float32))
    assert rows is None and skip == "[INFO] Key u2 has no voiced frame, skip."
    vad = np.zeros(50, np.float32)
    vad[[1, 5, 6, 40]] = 1.0
    rows, skip = utils.select_voiced("u3", feat, vad)
    assert skip is None and rows.shape == (4, 4) and rows.item is feat and rows.voiced.dtype == np.uint8 and rows.first == 0 and rows.count == 4
    with pytest.raises(ValueError):
        kaldi_io.VoicedRows(feat, np.ones(3, np.uint8))


def test_chunks_are_cut_in_post_selection_frames():
    """An utterance of 1000 raw frames of which 700 are voiced, --chunk-size 300: the pieces EmbeddingWindow hands to predict_batch are
    split_into_chunks(700, 300) in kept-frame indices, every piece naming the whole raw utterance and sharing its mask."""
    rs = np.random.RandomState(4)
    feat = rs.randn(1000, 4).astype(np.float32)
    vad = np.zeros(1000, np.float32)
    vad[rs.permutation(1000)[:700]] = 1.0
    rows, _ = utils.select_voiced("u", feat, vad)
    short, _ = utils.select_voiced("v", feat[:100], vad[:100])
    seen = []

    def predict_batch(pieces):
        seen.extend(pieces)
        return np.arange(len(pieces), dtype=np.float32)[:, None] * np.ones((1, 2), np.float32)

    res = utils.EmbeddingWindow(predict_batch, [rows, short], 300, False).results()
    chunks = utils.split_into_chunks(700, 300)
    assert len(chunks) > 1 and [(p.first, p.count) for p in seen[:-1]] == chunks
    assert all(p.item is feat and p.voiced is rows.voiced and p.shape == (n, 4) for p, (_, n) in zip(seen, chunks))
    assert seen[-1] is short and short.count == int(vad[:100].sum())
    assert [k for _, k in res] == [len(chunks), 1]
    weights = np.array([n for _, n in chunks], np.float64)
    assert np.allclose(res[0][0], (np.arange(len(chunks)) * weights).sum() / weights.sum())


def test_vad_table_ark_and_scp_by_key(tmp_path):
    """--vad ark: is read up front, --vad scp: is a table of rxfilenames read by key; neither has to follow the feature order."""
    rs = np.random.RandomState(5)
    vecs = {"b": rs.rand(7).astype(np.float32), "a": rs.rand(3).astype(np.float32), "c": rs.rand(5).astype(np.float32)}
    ark = str(tmp_path / "vad.ark")
    offsets = {}
    with open(ark, "wb") as f:
        for k, v in vecs.items():
            f.write((k + " ").encode())
            offsets[k] = f.tell()
            kaldi_io.write_vec_flt(f, v)
    scp = str(tmp_path / "vad.scp")
    with open(scp, "w") as f:
        for k in ("c", "a", "b"):
            f.write("%s %s:%d\n" % (k, ark, offsets[k]))
    assert [k for k, _ in kaldi_io.read_vec_flt_scp(scp)] == ["c", "a", "b"]
    for spec in ("ark:" + ark, "scp:" + scp, "scp,s,cs:" + scp):
        table = kaldi_io.VecFltTable(spec)
        for k in ("a", "c", "b"):
            assert np.array_equal(table.get(k), vecs[k]), (spec, k)
        assert table.get("missing") is None
    assert os.path.getsize(scp) > 0
