"""CPU checks of the scoring stage: the fp64 restatement (tests/score_ref.py) against literal per-element loops, the host metrics
(misc/scoring.py) against the existing pairwise EER and a brute-force detection-cost sweep, the trial reader, the driver's skip / order
rules on the host path, and the ABI table's new entries."""
import math
import os
import re

import numpy as np
import pytest

from tests import score_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_prepare_and_trials_match_per_element_loops():
    rs = np.random.RandomState(3)
    x = rs.randn(5, 9)
    x[2] = 0.0                                              # a zero row stays zero
    mean = rs.randn(7)
    got = R.prepare(x, d=7, mean=mean)
    for r in range(5):
        v = [x[r][c] - mean[c] for c in range(7)]
        ss = sum(a * a for a in v)
        for c in range(7):
            assert got[r][c] == pytest.approx(v[c] / math.sqrt(max(ss, 1e-12)), rel=1e-14, abs=1e-300)
    assert np.all(R.prepare(np.zeros((2, 4))) == 0.0)
    e, t = rs.randn(4, 6), rs.randn(3, 6)
    ei, ti = np.array([3, 3, 0, 2, 1]), np.array([2, 0, 0, 1, 2])
    es, ts = np.abs(rs.randn(4, 2)) + 0.1, np.abs(rs.randn(3, 2)) + 0.1
    raw, norm = R.trials(e, t, ei, ti), R.trials(e, t, ei, ti, es, ts)
    for j in range(5):
        s = sum(e[ei[j]][c] * t[ti[j]][c] for c in range(6))
        assert raw[j] == pytest.approx(s, rel=1e-14)
        want = 0.5 * ((s - es[ei[j]][0]) / es[ei[j]][1] + (s - ts[ti[j]][0]) / ts[ti[j]][1])
        assert norm[j] == pytest.approx(want, rel=1e-13)


@pytest.mark.parametrize("top_k", [1, 2, 3, 4, 6, 7, 20])
def test_top_k_stats_match_a_loop_including_a_cut_through_ties(top_k):
    """Row 0: the values 0.5 x 3 straddle the cut for top_k = 2 .. 4 (one 0.9 above them); row 1: all equal; top_k >= n takes every score."""
    scores = np.array([[0.5, -0.2, 0.9, 0.5, 0.1, 0.5, -0.7],
                       [0.3, 0.3, 0.3, 0.3, 0.3, 0.3, 0.3],
                       [-0.1, -0.9, -0.4, -0.3, -0.2, -0.8, -0.5]])
    got = R.top_k_stats(scores, top_k)
    for r in range(3):
        row = sorted(scores[r].tolist(), reverse=True)[:min(top_k, 7)]
        mean = sum(row) / len(row)
        var = sum((v - mean) ** 2 for v in row) / len(row)
        assert got[r][0] == pytest.approx(mean, rel=1e-14)
        assert got[r][1] == pytest.approx(math.sqrt(max(var, 1e-12)), rel=1e-12)
    assert got[1][1] == pytest.approx(1e-6)
    x, c = np.eye(3, 4), np.random.RandomState(0).randn(7, 4)
    assert np.array_equal(R.cohort_stats(x, c, top_k), R.top_k_stats(x @ c.T, top_k))


def test_pipeline_is_the_composition_of_the_three_ops():
    rs = np.random.RandomState(5)
    enrol, test, cohort = rs.randn(6, 8), rs.randn(5, 8), rs.randn(9, 8)
    centre = rs.randn(8)
    ei, ti = np.array([0, 5, 2]), np.array([4, 4, 1])
    got = R.score_pipeline(enrol, test, ei, ti, center=centre, cohort=cohort, top_k=4)
    for j in range(3):
        def unit(v):
            v = v - centre
            return v / np.linalg.norm(v)
        e, t = unit(enrol[ei[j]]), unit(test[ti[j]])
        co = np.array([unit(c) for c in cohort])
        s = float(e @ t)
        se, st = np.sort(co @ e)[::-1][:4], np.sort(co @ t)[::-1][:4]
        want = 0.5 * ((s - se.mean()) / se.std() + (s - st.mean()) / st.std())
        assert got[j] == pytest.approx(want, rel=1e-12)


def test_compute_eer_is_the_arithmetic_of_the_pairwise_function():
    from tf_kaldi_speaker_amd.misc import scoring, utils
    rs = np.random.RandomState(0)
    centres = rs.randn(6, 12) * 1.5
    emb = np.concatenate([c + rs.randn(7, 12) for c in centres])
    labels = np.repeat(np.arange(6), 7)
    unit = emb / np.sqrt((emb ** 2).sum(axis=1, keepdims=True) + 1e-12)
    iu = np.triu_indices(len(emb), k=1)
    scores, targets = (unit @ unit.T)[iu], (labels[iu[0]] == labels[iu[1]]).astype(np.float64)
    assert scoring.compute_eer(scores, targets) == utils.compute_cos_pairwise_eer(emb.copy(), labels)
    assert 0.0 < scoring.compute_eer(scores, targets) < 0.5


def test_compute_min_dcf_matches_a_sweep_over_every_threshold():
    from tf_kaldi_speaker_amd.misc import scoring
    rs = np.random.RandomState(2)
    targets = rs.rand(400) < 0.2
    scores = np.round(rs.randn(400) + 1.5 * targets, 1)                # rounded: many ties, across the two classes too
    assert scoring.MIN_DCF_PRESETS == {"minDCF08": (0.01, 10.0, 1.0), "minDCF10": (0.001, 1.0, 1.0)}
    for p, cm, cf in list(scoring.MIN_DCF_PRESETS.values()) + [(0.5, 1.0, 1.0), (0.05, 1.0, 1.0)]:
        best = min(cm * p, cf * (1 - p))                               # accept nothing (1, 0) and accept everything (0, 1) ...
        for thr in np.unique(scores):                                  # ... and every distinct score as the lowest accepted one
            p_miss = np.mean(scores[targets] < thr)
            p_fa = np.mean(scores[~targets] >= thr)
            best = min(best, cm * p * p_miss + cf * (1 - p) * p_fa)
        assert scoring.compute_min_dcf(scores, targets, p, cm, cf) == pytest.approx(best / min(cm * p, cf * (1 - p)), rel=1e-12)
    perfect = scoring.compute_min_dcf(np.array([2.0, 1.5, -1.0, -2.0]), np.array([1, 1, 0, 0]), 0.01, 10.0, 1.0)
    assert perfect == 0.0
    with pytest.raises(ValueError, match="at least one target and one nontarget"):
        scoring.compute_min_dcf(np.array([1.0, 2.0]), np.array([1, 1]), 0.01, 10.0, 1.0)


def test_read_trials(tmp_path):
    from tf_kaldi_speaker_amd.misc import scoring
    p = tmp_path / "trials"
    p.write_text("spk1-a spk2-b target\n\nspk1-a spk3-c nontarget\n   \nspk4-d spk1-a\n")
    assert scoring.read_trials(str(p)) == [("spk1-a", "spk2-b", True), ("spk1-a", "spk3-c", False), ("spk4-d", "spk1-a", None)]
    p.write_text("a b target\na c imposter\n")
    with pytest.raises(ValueError, match=r"trials:2: bad trial label 'imposter'"):
        scoring.read_trials(str(p))
    p.write_text("a b target extra\n")
    with pytest.raises(ValueError, match="got 4 columns"):
        scoring.read_trials(str(p))


def test_driver_host_path_skips_missing_keys_and_keeps_trial_order(tmp_path):
    """index_trials (what nnet/lib/score.py runs between reading and scoring): a trial with a missing key on either side is set aside, the
    others keep the order of the list and point at the rows of their tables; read_vectors reads ark and scp tables and refuses a ragged
    one; center_mean accumulates in fp64."""
    from tf_kaldi_speaker_amd.dataset import kaldi_io
    from tf_kaldi_speaker_amd.misc import scoring
    trials = [("e2", "t1", True), ("e9", "t1", False), ("e0", "t2", None), ("e2", "t7", True), ("e0", "t0", False), ("e2", "t1", True)]
    kept, ei, ti, skipped = scoring.index_trials(trials, ["e0", "e1", "e2"], ["t0", "t1", "t2"])
    assert kept == [trials[0], trials[2], trials[4], trials[5]] and skipped == [trials[1], trials[3]]
    assert ei.tolist() == [2, 0, 0, 2] and ti.tolist() == [1, 2, 0, 1] and ei.dtype == ti.dtype == np.int32
    keys = ["a", "b", "c"]
    kept, ei, ti, skipped = scoring.index_trials([("a", "c", None), ("c", "c", None), ("d", "a", None)], keys, keys)      # one table both sides
    assert ei.tolist() == [0, 2] and ti.tolist() == [2, 2] and len(skipped) == 1
    rs = np.random.RandomState(1)
    vecs = rs.randn(4, 5).astype(np.float32)
    ark, scp = str(tmp_path / "v.ark"), str(tmp_path / "v.scp")
    with open(ark, "wb") as f, open(scp, "w") as s:
        for i, v in enumerate(vecs):
            s.write("k%d %s:%d\n" % (i, ark, f.tell() + len("k%d " % i)))
            kaldi_io.write_vec_flt(f, v, key="k%d" % i)
    for spec in ("ark:" + ark, "scp:" + scp, ark):
        got_keys, got = scoring.read_vectors(spec)
        assert got_keys == ["k0", "k1", "k2", "k3"] and np.array_equal(got, vecs) and got.dtype == np.float32
    with open(ark, "ab") as f:
        kaldi_io.write_vec_flt(f, np.zeros(3, np.float32), key="short")
    with pytest.raises(ValueError, match="vector short has 3 dimensions"):
        scoring.read_vectors("ark:" + ark)
    big = (np.ones((3, 2)) * 1e8 + np.array([[0.0, 1.0], [2.0, 3.0], [4.0, 5.0]])).astype(np.float32)
    assert scoring.center_mean(big).dtype == np.float64 and np.array_equal(scoring.center_mean(big), big.astype(np.float64).mean(axis=0))


def test_header_and_ctypes_table_name_the_scoring_ops():
    from tf_kaldi_speaker_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "xvector_hip.h")).read(), flags=re.S)
    for name in ("xv_score_prepare", "xv_score_trials", "xv_score_cohort_stats", "xv_score_cohort_workspace_bytes"):
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(_lib.load(), name)
    assert _lib.ABI_VERSION == 3 and "#define XV_ABI_VERSION 3" in src
    lib = _lib.load()
    assert lib.xv_score_cohort_workspace_bytes(1, 1, 512) == 128 * 4 * 4                     # one 128-row tile, the cohort on the 16-byte grid
    assert lib.xv_score_cohort_workspace_bytes(129, 4097, 512) == 256 * 4100 * 4


def test_scoring_arguments_are_refused_by_name_before_any_launch():
    """The C entry points check their arguments on the host: no GPU is touched by a refused call."""
    import ctypes as C
    from tf_kaldi_speaker_amd import _lib
    lib = _lib.load()
    p = C.c_void_p(4096)

    def refused(rc, text):
        assert rc != 0 and text in lib.xv_last_error().decode(), lib.xv_last_error()
    refused(lib.xv_score_cohort_stats(None, p, 8, 4, p, 8, 4, 8, 0, p, p, 1 << 20), "top_k must be positive")
    refused(lib.xv_score_cohort_stats(None, p, 8, 4, p, 8, 0, 8, 2, p, p, 1 << 20), "n_cohort must be positive")
    refused(lib.xv_score_cohort_stats(None, p, 8, 4, p, 8, 4, 8, 2, p, p, 127 * 4 * 4), "at least one 128-row tile")
    refused(lib.xv_score_cohort_stats(None, p, 6, 4, p, 8, 4, 6, 2, p, p, 1 << 20), "both pitches must reach d rounded up to 4")
    refused(lib.xv_score_trials(None, p, 8, 4, p, 8, 4, 8, p, p, 3, p, None, p), "both be given or both be NULL")
    refused(lib.xv_score_prepare(None, p, 4, 8, 8, None, C.c_void_p(4096 + 16), 8), "x and y overlap")
    refused(lib.xv_score_prepare(None, p, 4, 8, 8, None, p, 12), "x and y overlap")                 # same base, another pitch: not in place
    refused(lib.xv_score_prepare(None, p, 4, 8, 6, None, C.c_void_p(1 << 20), 8), "a pitch is below d")
