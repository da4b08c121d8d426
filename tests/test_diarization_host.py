"""The host side of diarization (misc/diarization.py): speech segments, the window planner at its edges, the midpoint and merge rules of
the turns, RTTM files, the diarization error rate on hand-made turns, and Diarizer's refusals that come before any device.  No GPU."""
import logging
import os

import numpy as np
import pytest

from tf_kaldi_speaker_amd.misc import diarization as D

W, P, M = 150, 75, 50


def test_speech_segments():
    vad = np.array([0, 1, 1, 0, 0, 1, 1, 1, 0, 1], np.float32)
    assert D.speech_segments(vad) == [(1, 3), (5, 8), (9, 10)]
    assert D.speech_segments(vad, 2) == [(1, 3), (5, 8)] and D.speech_segments(vad, 4) == []
    assert D.speech_segments(np.ones(7)) == [(0, 7)] and D.speech_segments(np.zeros(7)) == [] and D.speech_segments([]) == []


def test_read_segments(tmp_path):
    path = os.path.join(str(tmp_path), "segments")
    with open(path, "w") as f:
        f.write("rec1-0001 rec1 0.00 3.25\n\nrec1-0002 rec1 4.5 9 1\nrec2-0001 rec2 1 2\n")
    assert D.read_segments(path) == [("rec1-0001", "rec1", 0.0, 3.25), ("rec1-0002", "rec1", 4.5, 9.0), ("rec2-0001", "rec2", 1.0, 2.0)]
    for bad, what in (("u r 1\n", "got 3 columns"), ("u r 2 2\n", "runs from 2 to 2"), ("u r -1 2\n", "runs from -1 to 2")):
        with open(path, "w") as f:
            f.write("a r 0 1\n" + bad)
        with pytest.raises(ValueError, match=":2: .*" + what):
            D.read_segments(path)


def test_window_planner_edges(caplog):
    assert D.subsegments(10, 10 + W, W, P, M) == [(10, 160)]                             # exactly one window: t_0 + W >= e stops at once
    assert D.subsegments(10, 10 + W + 1, W, P, M) == [(10, 160), (85, 161)]              # one frame more: a second window of W + 1 - P frames
    assert D.subsegments(0, 300, W, P, M) == [(0, 150), (75, 225), (150, 300)]           # the window that reaches the end is the last
    assert D.subsegments(0, 301, W, P, M) == [(0, 150), (75, 225), (150, 300), (225, 301)]
    # a last window shorter than M is dropped (it takes a period above W - M): [120, 160) has 40 < 50 frames ...
    assert D.subsegments(0, 160, W, 120, M) == [(0, 150)] and D.subsegments(0, 169, W, 120, M) == [(0, 150)]
    assert D.subsegments(0, 170, W, 120, M) == [(0, 150), (120, 170)]                    # ... one of exactly M is kept
    assert D.subsegments(0, 280, W, 120, M) == [(0, 150), (120, 270)]                    # [240, 280): 40 frames, dropped again
    # the first window is kept whatever its length, as long as the segment itself is not shorter than M
    assert D.subsegments(5, 5 + M, W, P, M) == [(5, 55)] and D.subsegments(5, 5 + 60, W, P, 70) == []
    with caplog.at_level(logging.INFO, logger="tf_kaldi_speaker_amd"):
        assert D.subsegments(5, 5 + M - 1, W, P, M) == []
    assert "49 frames, fewer than 50, dropped" in caplog.text
    # a period longer than the window leaves gaps; nothing overlaps the end
    assert D.subsegments(0, 500, 100, 200, 50) == [(0, 100), (200, 300), (400, 500)]
    with pytest.raises(ValueError, match="window and period must be positive"):
        D.subsegments(0, 100, 100, 0, 10)


def test_turns_midpoint_and_merge():
    subs = [(0.0, 1.5), (0.75, 2.25), (1.5, 3.0), (2.25, 3.75), (5.0, 6.5), (5.75, 7.25)]
    # overlaps are cut at their midpoints: 1.125, 1.875, 2.625 | 6.125; then equal neighbours that abut are merged
    assert D.rttm_turns(subs, [0, 0, 1, 1, 1, 0]) == [(0.0, 1.875, 0), (1.875, 3.75, 1), (5.0, 6.125, 1), (6.125, 7.25, 0)]
    assert D.rttm_turns(subs, [0, 1, 0, 1, 0, 0]) == [(0.0, 1.125, 0), (1.125, 1.875, 1), (1.875, 2.625, 0), (2.625, 3.75, 1), (5.0, 7.25, 0)]
    # one label across a gap stays two turns; the order of the input does not matter
    assert D.rttm_turns(subs, [2] * 6) == [(0.0, 3.75, 2), (5.0, 7.25, 2)]
    order = [3, 0, 5, 1, 4, 2]
    assert D.rttm_turns([subs[i] for i in order], [[0, 0, 1, 1, 1, 0][i] for i in order]) == D.rttm_turns(subs, [0, 0, 1, 1, 1, 0])
    assert D.rttm_turns([], []) == []
    with pytest.raises(ValueError, match="2 windows, 1 labels"):
        D.rttm_turns(subs[:2], [0])


def test_rttm_round_trip(tmp_path):
    path = os.path.join(str(tmp_path), "out.rttm")
    turns = {"recB": [(0.0, 1.875, 0), (1.875, 3.75, 1)], "recA": [(5.0, 6.125, 2)]}
    D.write_rttm(path, turns)
    lines = open(path).read().splitlines()
    assert lines == ["SPEAKER recB 0 0.000 1.875 <NA> <NA> 1 <NA> <NA>", "SPEAKER recB 0 1.875 1.875 <NA> <NA> 2 <NA> <NA>",
                     "SPEAKER recA 0 5.000 1.125 <NA> <NA> 3 <NA> <NA>"]
    back = D.read_rttm(path)
    assert list(back) == ["recB", "recA"]
    assert back["recB"] == [(0.0, 1.875, "1"), (1.875, 3.75, "2")] and back["recA"] == [(5.0, 6.125, "3")]
    with open(path, "a") as f:
        f.write("SPKR-INFO recA 0 <NA> <NA> <NA> unknown 3 <NA> <NA>\nSPEAKER recA 0 1.0\n")
    with pytest.raises(ValueError, match=":5: a SPEAKER line has at least 8 columns"):
        D.read_rttm(path)


def test_der_on_hand_made_turns():
    pytest.importorskip("scipy")
    ref = [(0.0, 4.0, "A"), (4.0, 10.0, "B")]
    assert D.der(ref, [(0.0, 4.0, 7), (4.0, 10.0, 3)]) == (0.0, 0.0, 0.0, 0.0)            # names do not matter
    # 1 s of B given to A's partner: confusion 1 / 10
    assert D.der(ref, [(0.0, 5.0, 0), (5.0, 10.0, 1)]) == (0.0, 0.0, 0.1, 0.1)
    # the last 2 s missed, 1.5 s of false alarm behind the end
    assert D.der(ref, [(0.0, 4.0, 0), (4.0, 8.0, 1), (10.0, 11.5, 1)]) == (0.2, 0.15, 0.0, 0.35)
    # one hypothesis speaker for everything: the smaller reference speaker is all confusion
    assert D.der(ref, [(0.0, 10.0, 0)]) == (0.0, 0.0, 0.4, 0.4)
    # three hypothesis speakers for two: the unmatched one is confusion
    assert D.der(ref, [(0.0, 4.0, 0), (4.0, 7.0, 1), (7.0, 10.0, 2)]) == (0.0, 0.0, 0.3, 0.3)
    # overlapped reference speech counts for the speaker who started first: C's 2 s inside A are not asked for
    assert D.der([(0.0, 4.0, "A"), (1.0, 3.0, "C"), (4.0, 10.0, "B")], [(0.0, 4.0, 0), (4.0, 10.0, 1)]) == (0.0, 0.0, 0.0, 0.0)
    with pytest.raises(ValueError, match="the reference holds no speech"):
        D.der([], [(0.0, 1.0, 0)])


def test_diarizer_refusals_before_any_device():
    class Scorer(object):
        torch = ops = device = None
        workspace_bytes = 1 << 20

    with pytest.raises(ValueError, match="exactly one of threshold and reco2num_spk"):
        D.Diarizer(Scorer())
    with pytest.raises(ValueError, match="exactly one of threshold and reco2num_spk"):
        D.Diarizer(Scorer(), threshold=0.1, reco2num_spk={})
    assert D.Diarizer(Scorer(), threshold=0.1).cluster({}) == {}
