"""Batched extraction, the code behind Trainer.predict_batch: one frame (predict_batch below: validate, plan, capacity, stage, batch
loop, torch.cat, inverse permutation, hand-back) over three sources of batches - plain_source (matrices and 'CM ' images as they are),
voiced_source (the same behind Engine.frontend) and device_source (kaldi_io.DeviceRows: features that are on the device already).  A source
stages what it needs once per call, in pinned uploads, and turns a batch of the plan into (x, rows) for Engine.forward_lengths.
The arithmetic that addresses device memory - byte offsets of archive blocks and masks, the inverse order - is in pure functions over
NumPy (stage_blocks, mask_table, inverse_order; validate beside them), tested without a GPU in tests/test_predict_plan.py: the kernels
check none of the index arrays they are handed."""
from collections import OrderedDict

import numpy as np
import torch

try:
    from ..misc.utils import plan_length_batches
    from ..dataset.kaldi_io import DeviceRows, PackedMatrix, VoicedRows
except (ImportError, ValueError):      # drop-in layout: PYTHONPATH=$TF_KALDI_ROOT
    from misc.utils import plan_length_batches
    from dataset.kaldi_io import DeviceRows, PackedMatrix, VoicedRows


# ------------------------------------------------------------------ host arithmetic (NumPy only: no device, no pinned memory, no engine)
def validate(items, voiced, dim, min_frames, cmn_window=0):
    """The refusals of predict_batch -> (kind, pieces, lengths).  kind: "device" (every item a DeviceRows), "voiced" (the front end is on:
    cmn_window > 0, `voiced`, or a VoicedRows among the items - pieces are then all VoicedRows: raw utterance, mask, range of kept
    frames) or "plain" (pieces = items).  lengths are what the network sees: the frames left after selection."""
    if any(isinstance(it, DeviceRows) for it in items):
        if voiced is not None or not all(isinstance(it, DeviceRows) for it in items):
            raise ValueError("predict_batch: DeviceRows items carry their own masks (voiced must be None) and do not mix with host items")
        kind, raw = "device", items
    else:
        if voiced is not None and len(voiced) != len(items):
            raise ValueError("predict_batch: %d voicing masks for %d items" % (len(voiced), len(items)))
        kind, raw = "plain", items
        if cmn_window > 0 or voiced is not None or any(isinstance(it, VoicedRows) for it in items):
            if voiced is not None and any(isinstance(it, VoicedRows) for it in items):
                raise ValueError("predict_batch: a VoicedRows item carries its own mask (voiced must be None)")
            items = [it if isinstance(it, VoicedRows) else VoicedRows(it, None if voiced is None else voiced[i]) for i, it in enumerate(items)]
            kind, raw = "voiced", [p.item for p in items]
    # every matrix must have the model's feature dimension: the GPU decoder takes the column stride from `dim`, not from the archive
    # header, so a mismatch would decode garbage (and read past the record) instead of failing; predict() rejects it through
    # Engine.forward, this is the same check for the batched path
    for i, it in enumerate(raw):
        if len(it.shape) != 2 or int(it.shape[1]) != dim:
            raise ValueError("predict_batch: item %d has shape %s, the model expects [frames, %d]" % (i, tuple(it.shape), dim))
    # an utterance shorter than the network's receptive field has no valid output frame (predict() refuses it in Engine.forward; here the
    # pooling would clamp to one frame that already sees zero padding); longer than max_frames cannot happen: the plan pads to the longest
    lengths = [int(it.shape[0]) for it in items]
    for i, t in enumerate(lengths):
        if t < min_frames:
            raise ValueError("predict_batch: item %d has %d frames, fewer than the network's receptive field (%d)" % (i, t, min_frames))
    if kind == "device" and len({it.batch.masks is None for it in items}) != 1:
        raise ValueError("predict_batch: DeviceRows items with and without masks do not mix")
    return kind, items, lengths


def stage_blocks(items):
    """Where the archive blocks of the items' PackedMatrix views go in one staging buffer -> (blocks in order of first appearance, their
    bases, the buffer's size, int64 byte offset of every item's image there).  A base is the running total rounded up to 16 bytes; an item
    lies at base + start of its block, a non-packed item gets 0."""
    base, blocks, total = {}, [], 0
    for it in items:
        if isinstance(it, PackedMatrix) and id(it.block) not in base:
            base[id(it.block)] = total
            blocks.append(it.block)
            total += (len(it.block) + 15) // 16 * 16
    offsets = [base[id(it.block)] + it.start if isinstance(it, PackedMatrix) else 0 for it in items]
    return blocks, [base[id(b)] for b in blocks], total, np.asarray(offsets, np.int64)


def mask_table(masks, raw):
    """The voicing masks of the pieces (uint8 arrays or None, in plan order; raw: their raw frame counts) back to back -> (int64 byte offset
    per piece, the bytes, their number).  One copy per mask object: the chunks of a long utterance share theirs.  A piece without a mask
    beside pieces with one points at a run of ones as long as the longest such utterance; no mask anywhere: nothing, all offsets 0."""
    if all(m is None for m in masks):
        return np.zeros(len(masks), np.int64), np.zeros(0, np.uint8), 0
    ones = np.ones(max([r for r, m in zip(raw, masks) if m is None] or [0]), np.uint8)
    masks = [ones if m is None else m for m in masks]
    at, parts, total = {}, [], 0
    for m in masks:
        if id(m) not in at:
            at[id(m)] = total
            parts.append(m)
            total += len(m)
    return np.asarray([at[id(m)] for m in masks], np.int64), np.concatenate(parts), total


def plan_order(plan):      # the items' indices in the order the plan's batches run them
    return [i for idx, _ in plan for i in idx]


def inverse_order(plan):      # inv: rows in plan order [inv] = rows in the caller's order
    flat = plan_order(plan)
    inv = np.empty(len(flat), np.int64)
    inv[flat] = np.arange(len(flat))
    return inv


# ------------------------------------------------------------------ the thin layer: pinned buffers and uploads
def _stage_host(items, dim, eng):
    """Host items for the GPU -> (items, uint8 device tensor of their archive blocks or None, stage_blocks' offsets).  'CM ' matrices stay
    where the reader cut them out: the archive blocks they are views of go to the GPU whole, once per call (a quarter of the fp32 bytes,
    no per-batch gather on the host); a batch is then a list of byte offsets for the on-GPU decode.  That decoder handles at most 128
    feature dimensions (one lane per column header); wider archives go through the host codec."""
    if dim > 128:
        items = [it.decode() if isinstance(it, PackedMatrix) else it for it in items]
    blocks, bases, total, offsets = stage_blocks(items)
    if not total:
        return items, None, offsets
    host = torch.empty(total, dtype=torch.uint8, pin_memory=True)
    for blk, o in zip(blocks, bases):
        host.numpy()[o:o + len(blk)] = np.frombuffer(blk, np.uint8)
    return items, host.to(eng.device, non_blocking=True), offsets


def _upload_table(rows, eng, tail=None):
    """The metadata of every batch - int64 rows [k, pieces], in plan order - and a run of bytes behind them (the masks) in ONE pinned
    upload: a pageable host -> device copy per batch makes the host wait for the stream (the previous batch's forward), i.e. host and GPU
    work would take turns instead of overlapping.  -> (int64 device tensor [k, pieces], uint8 device tensor or None)"""
    rows = np.asarray(rows, np.int64)
    head, extra = rows.size * 8, 0 if tail is None else len(tail)
    meta = torch.empty(head + extra, dtype=torch.uint8, pin_memory=True)
    meta.numpy()[:head].view(np.int64)[:] = rows.reshape(-1)
    if extra:
        meta.numpy()[head:] = tail
    dev = meta.to(eng.device, non_blocking=True)
    return dev[:head].view(torch.int64).view(rows.shape), dev[head:] if extra else None


def _padded(items, idx, t, dim):      # a batch that is not all 'CM ': its matrices in a zero-padded host block [len(idx), t, dim]
    host = np.zeros((len(idx), t, dim), np.float32)
    for j, i in enumerate(idx):
        m = items[i].decode() if isinstance(items[i], PackedMatrix) else np.asarray(items[i], np.float32)
        host[j, :m.shape[0]] = m
    return host


# ------------------------------------------------------------------ the sources
# source(eng, pieces, lengths, flat, dim, cmn_window) stages what the call needs (flat: plan_order) and returns batch(idx, t, sl) -> (x, rows)
# of the plan's batch (idx, t), sl being the batch's slice of the plan order.
def plain_source(eng, items, lengths, flat, dim, cmn_window):
    """Host float32 matrices and / or PackedMatrix, no front end.  Staged: the archive blocks, and per piece its byte offset and frames."""
    items, packed, offsets = _stage_host(items, dim, eng)
    table, _ = _upload_table([offsets[flat], np.asarray(lengths)[flat]], eng)
    offsets, rows = table[0], table[1].to(torch.int32)

    def batch(idx, t, sl):
        if all(isinstance(items[i], PackedMatrix) for i in idx):
            return eng.decode_packed(packed, offsets[sl], rows[sl], t)
        return _padded(items, idx, t, dim), rows[sl]      # (Engine.forward_lengths uploads the block)
    return batch


def voiced_source(eng, pieces, lengths, flat, dim, cmn_window):
    """The same items as RAW features behind Engine.frontend (cmn_window > 0, voiced=, VoicedRows): pieces are VoicedRows and a length
    counts kept frames.  The front end's arguments ride in the metadata upload: per piece the byte offset of its image, the byte offset
    of its mask, its raw frame count and the range of kept frames it covers, then the masks themselves (mask_table)."""
    items, packed, offsets = _stage_host([p.item for p in pieces], dim, eng)
    raw = [int(items[i].shape[0]) for i in flat]
    mask_at, masks, _ = mask_table([pieces[i].voiced for i in flat], raw)
    table, masks = _upload_table([offsets[flat], mask_at, raw, [pieces[i].first for i in flat], [pieces[i].count for i in flat]], eng, masks)
    offsets, mask_at = table[0], table[1]
    fe = table[2:5].to(torch.int32)      # raw rows, first, count

    def batch(idx, t, sl):
        # the raw batch is as long as its longest RAW utterance (the plan's t counts kept frames); host matrices take the same kernel
        t_raw = max(int(items[i].shape[0]) for i in idx)
        if all(isinstance(items[i], PackedMatrix) for i in idx):
            xr, _ = eng.decode_packed(packed, offsets[sl], fe[0, sl], t_raw)
        else:
            xr = torch.from_numpy(_padded(items, idx, t_raw, dim)).to(eng.device)
        return eng.frontend(xr, fe[0, sl], cmn_window, masks, mask_at[sl] if masks is not None else None, fe[1, sl], fe[2, sl], t)
    return batch


def device_source(eng, items, lengths, flat, dim, cmn_window):
    """kaldi_io.DeviceRows (extract.py's wav mode): the pieces are planned by their kept length exactly as host items are - whichever
    DeviceBatch they sit in - and a batch of the plan gathers its utterances' raw rows on the device (index_select, cut at the batch's
    longest raw utterance: the padded block a host batch would upload) and runs Engine.frontend on them with the DeviceBatches' masks,
    so the front end and the network see what they see when the same features come from an archive.  Nothing but the embeddings
    leaves the device."""
    sources, where = [], {}      # the DeviceBatches of this call, in order of appearance
    for it in items:
        if id(it.batch) not in where:
            where[id(it.batch)] = len(sources)
            sources.append(it.batch)
    src_of = [where[id(it.batch)] for it in items]
    # the sources' frame counts and masks back to back (a copy only when a call spans several sources: the end of a feature window)
    row_base = np.concatenate([[0], np.cumsum([len(src.frames) for src in sources])])
    mask_base = np.concatenate([[0], np.cumsum([len(src.frames) * int(src.x.shape[1]) for src in sources])])
    rows_all = sources[0].rows if len(sources) == 1 else torch.cat([src.rows for src in sources])
    masks_all = None
    if sources[0].masks is not None:
        masks_all = sources[0].masks.reshape(-1) if len(sources) == 1 else torch.cat([src.masks.reshape(-1) for src in sources])
    # per piece, in plan order: its utterance's index in its source and among all sources, the byte offset of its mask, first, count
    table, _ = _upload_table([[items[i].index for i in flat], [row_base[src_of[i]] + items[i].index for i in flat],
                              [mask_base[src_of[i]] + items[i].index * int(items[i].batch.x.shape[1]) for i in flat],
                              [items[i].first for i in flat], [items[i].count for i in flat]], eng)
    range_dev = table[3:5].to(torch.int32)

    def batch(idx, t, sl):
        t_raw = max(items[i].batch.frames[items[i].index] for i in idx)
        here = sorted({src_of[i] for i in idx})
        if len(here) == 1:
            xr = sources[here[0]].x[:, :t_raw].index_select(0, table[0, sl])
        else:
            xr = torch.zeros((len(idx), t_raw, dim), dtype=torch.float32, device=eng.device)
            for g in here:
                pos = torch.as_tensor([k for k, i in enumerate(idx) if src_of[i] == g], dtype=torch.int64, device=eng.device)
                tg = min(t_raw, int(sources[g].x.shape[1]))
                xr[pos, :tg] = sources[g].x[:, :tg].index_select(0, table[0, sl].index_select(0, pos))
        return eng.frontend(xr, rows_all.index_select(0, table[1, sl]), cmn_window, masks_all, table[2, sl] if masks_all is not None else None,
                            range_dev[0, sl], range_dev[1, sl], t)
    return batch


SOURCES = {"plain": plain_source, "voiced": voiced_source, "device": device_source}


# ------------------------------------------------------------------ the frame
class _PendingEmbeddings(object):
    """Embeddings of Trainer.predict_batch(..., return_device=True): still on the GPU, in batch order; cpu().numpy() reads them back and
    puts them into the caller's order."""

    def __init__(self, dev, inv):
        # the read-back is enqueued NOW, behind this window's forward passes, into pinned memory, and an event marks its end: numpy()
        # then waits for that event only.  (A dev.cpu() at read time queues behind whatever the caller has enqueued since - the next
        # window's decode and forward passes in extract.py - so host post-processing and GPU work took turns)
        self.inv = inv
        self.host = torch.empty(dev.shape, dtype=dev.dtype, pin_memory=True)
        self.host.copy_(dev, non_blocking=True)
        self.done = torch.cuda.Event()
        self.done.record(torch.cuda.current_stream(dev.device))
        self.dev = dev          # (kept alive until the copy has run)

    def cpu(self):
        return self

    def numpy(self):
        self.done.synchronize()
        self.dev = None
        return self.host.numpy()[self.inv]


def predict_batch(trainer, items, return_device=False, cmn_window=0, voiced=None):
    """Trainer.predict_batch (its docstring is the contract) on a trainer whose model is loaded."""
    if len(items) == 0:
        return np.zeros((0, 0), np.float32)
    cmn_window, node = int(cmn_window), trainer.params.embedding_node
    kind, items, lengths = validate(items, voiced, trainer.dim, trainer.engine.min_frames, cmn_window)
    plan = plan_length_batches(lengths, trainer.PREDICT_ROWS, trainer.PREDICT_CHUNKS)
    trainer._ensure_capacity(max(len(idx) for idx, _ in plan), max(t for _, t in plan), rows=max(trainer.PREDICT_ROWS, max(len(idx) * t for idx, t in plan)))
    eng = trainer.engine      # (the engine that has the capacity)
    batch = SOURCES[kind](eng, items, lengths, plan_order(plan), trainer.dim, cmn_window)
    outs, cursor = [], 0
    for idx, t in plan:
        x, rows = batch(idx, t, slice(cursor, cursor + len(idx)))
        cursor += len(idx)
        eng.forward_lengths(x, rows)
        emb = eng.endpoint(node)
        if emb.shape[0] != len(idx):
            raise ValueError("predict_batch: embedding node %s is a frame-level endpoint (%d rows for %d utterances)" % (node, emb.shape[0], len(idx)))
        outs.append(emb)
    dev = torch.cat(outs, dim=0)
    inv = inverse_order(plan)
    if return_device:
        # nothing here waits for the GPU (the permutation back to the caller's order is applied on the host after the read-back: an
        # index tensor uploaded from pageable memory would have made this call wait for the whole window's forward passes)
        return _PendingEmbeddings(dev, inv)
    emb = dev.cpu().numpy()[inv]
    trainer.endpoints = OrderedDict([(node, emb)])
    return emb
