"""The host arithmetic of batched extraction (tf_kaldi_speaker_amd/model/predict.py) without a GPU: where archive blocks and voicing masks
go in their staging buffers, the inverse of a batch plan, and the refusals of Trainer.predict_batch with their texts.  The kernels behind
these arrays check none of them: a wrong byte offset is an out-of-bounds read on the device."""
import numpy as np
import pytest

from tf_kaldi_speaker_amd.dataset.kaldi_io import DeviceRows, PackedMatrix, VoicedRows
from tf_kaldi_speaker_amd.misc.utils import plan_length_batches
from tf_kaldi_speaker_amd.model import predict as P


def _view(block, start, rows, cols):      # a PackedMatrix that is a view of `block` from byte `start` on
    size = PackedMatrix.HEADER + 8 * cols + cols * rows
    return PackedMatrix(rows, cols, memoryview(block)[start:start + size], block=block, start=start)


def test_block_staging_rounds_bases_to_16_and_offsets_follow_the_views():
    a, b = bytes(range(17)), bytes(range(100, 132))      # 17 and 32 bytes: the second base is 32 only if the first block is rounded up
    first, second = _view(a, 0, 0, 0), _view(a, 1, 0, 0)               # two views of one block
    third = _view(b, 7, 1, 1)
    items = [first, np.zeros((3, 1), np.float32), third, second]
    blocks, bases, total, offsets = P.stage_blocks(items)
    assert [id(x) for x in blocks] == [id(a), id(b)] and bases == [0, 32] and total == 64
    assert offsets.dtype == np.int64 and offsets.tolist() == [0 + 0, 0, 32 + 7, 0 + 1]
    # every image lies inside the staged bytes, where the block's own bytes will be
    for it, o in zip(items, offsets):
        if isinstance(it, PackedMatrix):
            assert o + len(it.payload) <= bases[[id(x) for x in blocks].index(id(it.block))] + len(it.block) <= total
    assert P.stage_blocks([items[1]])[1:3] == ([], 0) and P.stage_blocks([items[1]])[3].tolist() == [0]
    blocks, bases, total, offsets = P.stage_blocks([third, first])                  # first appearance decides the order
    assert [id(x) for x in blocks] == [id(b), id(a)] and bases == [0, 32] and total == 64 and offsets.tolist() == [7, 32]


def test_mask_table_shares_one_copy_per_mask_and_one_run_of_ones():
    long_mask = (np.arange(40) % 3 != 0).astype(np.uint8)
    other = np.ones(9, np.uint8)
    other[4] = 0
    # two chunks of one utterance (the same mask object), a maskless piece of 23 raw frames, another utterance, a maskless piece of 17
    at, data, total = P.mask_table([long_mask, None, long_mask, other, None], [40, 23, 40, 9, 17])
    assert at.dtype == np.int64 and at[0] == at[2] == 0
    assert at[1] == at[4] == 40 and at[3] == 40 + 23 and total == 40 + 23 + 9 == len(data)
    assert data.dtype == np.uint8 and np.array_equal(data, np.concatenate([long_mask, np.ones(23, np.uint8), other]))
    # an equal mask that is another object is another copy: identity, not value, says "the same utterance"
    at, data, total = P.mask_table([long_mask, long_mask.copy()], [40, 40])
    assert at.tolist() == [0, 40] and total == 80
    # every piece has a mask: no run of ones
    at, data, total = P.mask_table([other, long_mask], [9, 40])
    assert at.tolist() == [0, 9] and total == 49 and np.array_equal(data, np.concatenate([other, long_mask]))
    # no mask at all (sliding-window CMN only): nothing to upload
    at, data, total = P.mask_table([None, None, None], [30, 50, 16])
    assert at.tolist() == [0, 0, 0] and total == 0 and len(data) == 0


def test_inverse_order_restores_the_input_order():
    lengths = [30, 50, 30, 50, 16]
    for max_rows, max_chunks in ((49152, 128), (100, 2), (50, 1)):      # one batch; batches of two; one utterance each
        plan = plan_length_batches(lengths, max_rows, max_chunks, min_rows=0)
        flat = P.plan_order(plan)
        assert sorted(flat) == list(range(5)) and [lengths[i] for i in flat] == sorted(lengths, reverse=True)
        inv = P.inverse_order(plan)
        assert inv.dtype == np.int64 and np.array_equal(inv[flat], np.arange(5))
        rows_in_plan_order = np.asarray([[10 * i, lengths[i]] for i in flat])
        assert np.array_equal(rows_in_plan_order[inv], [[10 * i, n] for i, n in enumerate(lengths)])


class _Batch(object):      # what validate reads of a kaldi_io.DeviceBatch
    def __init__(self, masks):
        self.masks = masks


class _Rows(DeviceRows):      # a DeviceRows without tensors: shape, count, batch
    def __init__(self, batch, count, dim=30):
        self.batch, self.count, self._dim = batch, count, dim

    @property
    def shape(self):
        return (self.count, self._dim)


def test_validate_refuses_with_the_texts_of_predict_batch():
    ok, short, narrow = np.zeros((40, 30), np.float32), np.zeros((14, 30), np.float32), np.zeros((40, 24), np.float32)
    mask = np.ones(40, np.uint8)
    masked, bare = _Batch(object()), _Batch(None)
    mixing = r"predict_batch: DeviceRows items carry their own masks \(voiced must be None\) and do not mix with host items"
    for items, voiced, text in (
            ([_Rows(bare, 40), ok], None, mixing),
            ([_Rows(bare, 40)], [mask], mixing),
            ([ok, ok], [mask], "predict_batch: 1 voicing masks for 2 items"),
            ([VoicedRows(ok, mask), ok], [mask, mask], r"predict_batch: a VoicedRows item carries its own mask \(voiced must be None\)"),
            ([ok], [mask[:39]], "VoicedRows: 39 voicing decisions for 40 frames"),
            ([ok, narrow], None, r"predict_batch: item 1 has shape \(40, 24\), the model expects \[frames, 30\]"),
            ([ok, np.zeros(40, np.float32)], None, r"predict_batch: item 1 has shape \(40,\), the model expects \[frames, 30\]"),
            ([VoicedRows(narrow)], None, r"predict_batch: item 0 has shape \(40, 24\), the model expects \[frames, 30\]"),
            ([_Rows(bare, 40, dim=24)], None, r"predict_batch: item 0 has shape \(40, 24\), the model expects \[frames, 30\]"),
            ([ok, short], None, r"predict_batch: item 1 has 14 frames, fewer than the network's receptive field \(15\)"),
            ([VoicedRows(ok, mask, 0, 14)], None, r"predict_batch: item 0 has 14 frames, fewer than the network's receptive field \(15\)"),
            ([_Rows(bare, 40), _Rows(bare, 14)], None, r"predict_batch: item 1 has 14 frames, fewer than the network's receptive field \(15\)"),
            ([_Rows(bare, 40), _Rows(masked, 40)], None, "predict_batch: DeviceRows items with and without masks do not mix")):
        with pytest.raises(ValueError, match="^" + text + "$"):
            P.validate(items, voiced, 30, 15)


def test_validate_names_the_source_and_counts_kept_frames():
    ok, mask = np.zeros((40, 30), np.float32), (np.arange(40) % 2).astype(np.uint8)
    kind, pieces, lengths = P.validate([ok, ok[:15]], None, 30, 15)
    assert kind == "plain" and pieces[0] is ok and lengths == [40, 15]
    kind, pieces, lengths = P.validate([ok], None, 30, 15, cmn_window=300)      # the front end without a mask: every frame is kept
    assert kind == "voiced" and isinstance(pieces[0], VoicedRows) and pieces[0].item is ok and pieces[0].voiced is None and lengths == [40]
    kind, pieces, lengths = P.validate([ok, ok], [mask, None], 30, 15)
    assert kind == "voiced" and lengths == [20, 40] and np.array_equal(pieces[0].voiced, mask)
    chunk = VoicedRows(ok, mask, 2, 16)
    kind, pieces, lengths = P.validate([chunk, ok], None, 30, 15)
    assert kind == "voiced" and pieces[0] is chunk and lengths == [16, 40]
    rows = [_Rows(_Batch(None), 33), _Rows(_Batch(None), 15)]
    assert P.validate(rows, None, 30, 15) == ("device", rows, [33, 15])
