"""Diarization error counts on a real MI355X: xv_diar_confusion through ops.diar_frames / ops.diar_confusion against
tests/diar_eval_ref.py.  Every output is an integer, so the counts are asserted EQUAL: recordings of 1, 63, 64, 65, 1000 and 100 003 frames
(less than a wave, a wave, more than a workgroup's stride), 1 and 32 reference speakers, 1, 256 and 257 clusters - the last is not counted
and says so -, a recording without a scored frame, windows that leave frames to nobody, all in one call of several cuts."""
import numpy as np
import pytest

from tests import diar_eval_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# (frames, reference speakers, windows, share of the frames that is scored)
RECORDINGS = [(1, 1, 1, 1.0), (63, 1, 3, 0.9), (64, 32, 40, 0.9), (65, 32, 300, 0.9), (1000, 5, 300, 0.8), (100003, 32, 300, 0.9), (500, 3, 10, 0.0)]
CLUSTERS = (1, 7, 256, 257)      # of a cut, in the recordings with that many windows: the others have a cluster per window


def _ops():
    import torch
    from tf_kaldi_speaker_amd import ops
    return torch, ops


_WORLD = {}


def _world():
    """The reference of RECORDINGS, the labels of every cut, and the restatement's counts; built once, read only."""
    if not _WORLD:
        rs = np.random.RandomState(23)
        masks, flags, owners, labels = [], [], [], []
        for frames, speakers, n, share in RECORDINGS:
            talk = rs.rand(frames, speakers) < min(0.6, 1.5 / speakers)      # silence, one speaker and overlapped speech all occur
            masks.append((talk.astype(np.uint64) << np.arange(speakers, dtype=np.uint64)[None, :]).sum(axis=1).astype(np.uint32))
            flags.append((rs.rand(frames) < share).astype(np.uint8))
            own = np.sort(rs.randint(0, n, frames)).astype(np.int32)      # ascending windows, some of them without a frame
            own[rs.rand(frames) < 0.15] = -1                              # ... and frames in the gaps between windows
            owners.append(own)
            per_cut = []
            for k in CLUSTERS:
                lab = rs.randint(0, min(k, n), n).astype(np.int32)
                lab[:min(k, n)] = np.arange(min(k, n))      # every cluster has a window
                per_cut.append(lab)
            labels.append(np.stack(per_cut))
        for a in masks + flags + owners + labels:
            a.setflags(write=False)
        clusters = np.asarray([[min(k, n) for _, _, n, _ in RECORDINGS] for k in CLUSTERS], np.int64)
        want = [[R.confusion(masks[i], flags[i], owners[i], labels[i][c], RECORDINGS[i][1], clusters[c, i]) if clusters[c, i] <= 256 else None
                 for i in range(len(RECORDINGS))] for c in range(len(CLUSTERS))]
        _WORLD.update(masks=masks, flags=flags, owners=owners, labels=labels, clusters=clusters, want=want)
    return _WORLD


def _frames(ops, w, pick):
    frames, speakers, n, _ = zip(*[RECORDINGS[i] for i in pick])
    return ops.diar_frames(np.concatenate([w["masks"][i] for i in pick]), np.concatenate([w["flags"][i] for i in pick]),
                           np.concatenate([w["owners"][i] for i in pick]), frames, n, speakers, DEV)


def _check(w, pick, cuts, got):
    totals, overlap, offsets, status = got[0].cpu().numpy(), got[1].cpu().numpy(), got[2], got[3].cpu().numpy()
    assert totals.dtype == np.int64 and overlap.dtype == np.int32 and status.dtype == np.int32
    used = 0
    for c, cut in enumerate(cuts):
        for j, i in enumerate(pick):
            want, speakers, k = w["want"][cut][i], RECORDINGS[i][1], int(w["clusters"][cut, i])
            if want is None:
                assert status[c, j] == 1 and totals[c, j].tolist() == [0, 0, 0], (cut, i)      # not counted, and it says so
                continue
            assert status[c, j] == 0 and totals[c, j].tolist() == list(want[:3]), (cut, i)
            assert offsets[c, j] == used
            assert np.array_equal(overlap[used:used + speakers * k].reshape(speakers, k), want[3]), (cut, i)
            used += speakers * k
    assert used == overlap.size


def test_counts_equal_the_restatement_for_every_recording_and_cut_in_one_call():
    torch, ops = _ops()
    w = _world()
    pick, cuts = list(range(len(RECORDINGS))), list(range(len(CLUSTERS)))
    reference = _frames(ops, w, pick)
    labels = torch.from_numpy(np.concatenate(w["labels"], axis=1)).to(DEV)
    got = ops.diar_confusion(reference, labels, w["clusters"])
    _check(w, pick, cuts, got)
    # the unscored recording holds zeros, the single frame its one count
    assert got[0][:, 6].abs().sum().item() == 0 and w["want"][0][5][0] > 100000
    # clusters as a device tensor (what ahc_cut hands over), and the same bytes from a second call
    again = ops.diar_confusion(reference, labels, torch.from_numpy(w["clusters"].astype(np.int32)).to(DEV))
    assert torch.equal(again[0], got[0]) and torch.equal(again[1], got[1]) and torch.equal(again[3], got[3]) and np.array_equal(again[2], got[2])


@pytest.mark.parametrize("pick,cuts", [([0], [0]), ([5], [2]), ([3, 1], [3, 1, 0]), ([6, 2, 4], [1])])
def test_subsets_of_recordings_and_cuts(pick, cuts):
    """A recording's counts do not depend on its place in a call, nor on the other cuts."""
    torch, ops = _ops()
    w = _world()
    labels = torch.from_numpy(np.ascontiguousarray(np.concatenate([w["labels"][i] for i in pick], axis=1)[cuts])).to(DEV)
    _check(w, pick, cuts, ops.diar_confusion(_frames(ops, w, pick), labels, w["clusters"][np.ix_(cuts, pick)]))


def test_entries_out_of_range_are_not_counted_and_refusals():
    torch, ops = _ops()
    w = _world()
    reference = _frames(ops, w, [2, 4])
    labels = np.concatenate([w["labels"][2], w["labels"][4]], axis=1)[:2].copy()
    labels[1, 40:] = 7      # recording 4's cut 1 has 7 clusters: 0 .. 6
    clusters = w["clusters"][np.ix_([0, 1], [2, 4])].copy()
    clusters[0, 0] = -1      # what ahc_cut leaves for a recording it skipped
    _, _, _, status = ops.diar_confusion(reference, torch.from_numpy(labels).to(DEV), clusters)
    assert status.cpu().numpy().tolist() == [[-1, 0], [0, -1]]
    with pytest.raises(ValueError, match="^diar_confusion: labels must be a contiguous int32 \\[cuts, 340\\] tensor$"):
        ops.diar_confusion(reference, torch.zeros(2, 339, dtype=torch.int32, device=DEV), clusters)
    with pytest.raises(ValueError, match="^diar_confusion: clusters must be an integer \\[2, 2\\] array$"):
        ops.diar_confusion(reference, torch.from_numpy(labels).to(DEV), clusters[:1])
    one = lambda **kw: ops.diar_frames(**dict(dict(ref_mask=np.zeros(4, np.uint32), scored=np.ones(4, np.uint8), frame_window=np.zeros(4, np.int32), frames=[4], n=[2],
                                                  speakers=[1], device=DEV), **kw))
    assert one().frames.tolist() == [4]
    with pytest.raises(ValueError, match="^diar_frames: recording 0 has 33 reference speakers, 1 .. 32 are taken$"):
        one(speakers=[33])
    with pytest.raises(IndexError, match="^diar_frames: recording 0: frame_window holds a value outside -1 .. 1$"):
        one(frame_window=np.asarray([0, 1, 2, -1], np.int32))
    with pytest.raises(ValueError, match="^diar_frames: recording 0: ref_mask has a bit at or above its 1 speakers$"):
        one(ref_mask=np.asarray([0, 1, 2, 0], np.uint32))
    with pytest.raises(ValueError, match="^diar_frames: ref_mask must be a uint32 array of 4 frames$"):
        one(ref_mask=np.zeros(4, np.int32))
