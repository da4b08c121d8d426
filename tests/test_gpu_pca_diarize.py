"""The per-recording PCA of PLDA scoring through the layers above the op, on a real MI355X: BackendScorer.prepare_pca, Diarizer(target_energy=)
and nnet/lib/diarize.py --target-energy, against the NumPy restatement (tests/pca_plda_ref.py scores in double -> tests/ahc_ref.py in
double).

The device's scores differ from the restatement's by fp32 rounding (tests/test_gpu_pca_plda.py bounds it), so equal labels are asserted only
where the result cannot depend on that, in one of two ways (delta = the largest difference seen between the two score matrices; an average
of scores that are each within delta of the restatement's is within delta of its average, so 2 delta decides and 4 delta is asserted):
_margin() replays the double run and returns the smallest distance of a decision from flipping - the best average against every other
pair's at each merge, and against the threshold where the run stops: above it the merge order itself is the same; _partition_gap() is the
check tests/test_gpu_diarize.py uses - every score inside a cluster of the restatement's result above every score across two of them:
then every average inside is above every average across, whatever the order of the merges, and merging down to that number of clusters
ends in that partition."""
import os

import numpy as np
import pytest

from tests import ahc_ref as A
from tests import pca_plda_ref as P
from tests import test_gpu_diarize as TD
from tests import test_gpu_vbx_diarize as TV

pytestmark = pytest.mark.gpu

DEV = TD.DEV


def _margin(s, threshold=0.0, target=0):
    """The smallest distance from flipping over the decisions of the double run of average linkage on s (the arithmetic of tests/ahc_ref.py)."""
    s = np.asarray(s, np.float64)
    n = s.shape[0]
    t = A.upper_symmetric(s, np.float64)
    size, active = np.ones(n), np.ones(n, bool)
    margin, count, stop_at = np.inf, n, max(int(target), 1)
    while count > stop_at:
        pair = np.triu(np.outer(active, active), 1)
        avg = np.where(pair, t / np.outer(size, size), -np.inf)
        a, b = divmod(int(np.argmax(avg)), n)
        if target == 0:
            margin = min(margin, abs(avg[a, b] - threshold))
            if not avg[a, b] >= threshold:
                break
        rest = pair.copy()
        rest[a, b] = False
        if rest.any():
            margin = min(margin, avg[a, b] - avg[rest].max())
        others = active.copy()
        others[[a, b]] = False
        t[a, others] = t[a, others] + t[b, others]
        t[others, a] = t[a, others]
        size[a] += size[b]
        active[b] = False
        count -= 1
    return margin


def _partition_gap(s, labels):
    """min of the scores of two rows of one cluster minus max of the scores across clusters, over the upper triangle."""
    labels = np.asarray(labels)
    same = np.equal.outer(labels, labels)
    upper = np.triu(np.ones_like(same), 1)
    if not (same & upper).any() or not (~same & upper).any():
        return np.inf
    return float(s[same & upper].min() - s[~same & upper].max())


def _decided(ref, labels, delta, **stop):
    return max(_margin(ref, **stop), _partition_gap(ref, labels) if stop.get("target") else -np.inf) >= 4 * delta


def _reference_scores(scorer, x, target):
    """The restatement's scores of the raw vectors x: the chain's unit-length fp32 rows (the op's input), then everything in double."""
    unit = scorer.chain.unit(scorer.torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(DEV)).cpu().numpy()[:, :scorer.dim]
    w, b = P.covariances(scorer.backend.plda)
    assert P.qualifies(unit, target)
    return P.scores(unit, w, b, scorer.backend.plda["mean"], target), P.estimate(unit, w, b, scorer.backend.plda["mean"], target)["p"]


def test_diarizer_with_target_energy_gives_the_restatements_labels():
    from tf_kaldi_speaker_amd.misc import backend as B
    from tf_kaldi_speaker_amd.misc import diarization as D
    backend, recos = TD._world()
    scorer = B.BackendScorer(backend, "plda", DEV)
    emb = {k: x for k, (x, _) in recos.items()}
    speakers = {k: int(who.max()) + 1 for k, (_, who) in recos.items()}
    for target in (0.5, 0.9):
        own = scorer.prepare_pca(list(emb.values()), target)
        want, kept = {}, {}
        for (k, x), (prepared, model) in zip(emb.items(), own):
            ref, p = _reference_scores(scorer, x, target)
            got = scorer.dense(prepared, model=model).cpu().numpy()
            delta = float(np.abs(got - ref).max())
            want[k] = A.cluster(ref, target=speakers[k], dtype=np.float64)[0].tolist()
            print("target %g recording %s: p = %d of %d, scores of size %.3g, device - restatement %.3e, smallest merge margin %.3e, partition gap %.3e"
                  % (target, k, p, scorer.dim, np.abs(ref).max(), delta, _margin(ref, target=speakers[k]), _partition_gap(ref, want[k])))
            assert model is not None and model[0] == p and _decided(ref, want[k], delta, target=speakers[k])
            kept[k] = p
        diar = D.Diarizer(scorer, reco2num_spk=speakers, target_energy=target)
        got = diar.cluster(emb)
        assert list(got) == list(emb) and {k: v.tolist() for k, v in got.items()} == want and diar.pca_report == kept
        # one recording per call: a workspace that holds the largest recording only gives the same labels and the same report
        dim4 = 12
        cost = lambda n: 4 * (n * ((n + 3) // 4 * 4) + n * n) + 4 * n * dim4 + scorer.ops.backend_pca_plda_workspace_bytes(1, scorer.dim) + 4 * dim4 * (dim4 + 8)
        small = B.BackendScorer(backend, "plda", DEV, workspace_bytes=cost(61))
        one = D.Diarizer(small, reco2num_spk=speakers, target_energy=target)
        assert {k: v.tolist() for k, v in one.cluster(emb).items()} == want and one.pca_report == kept
        small.workspace_bytes -= 4
        with pytest.raises(ValueError, match="recording recC needs %d bytes of scores, the workspace holds %d" % (cost(61), cost(61) - 4)):
            one.cluster(emb)


def test_no_target_energy_is_todays_clusterer_bit_for_bit():
    import torch
    from tf_kaldi_speaker_amd.misc import backend as B
    from tf_kaldi_speaker_amd.misc import diarization as D
    backend, recos = TD._world()
    scorer = B.BackendScorer(backend, "plda", DEV)
    emb = {k: x for k, (x, _) in recos.items()}
    emb["one"] = recos["recA"][0][:1]      # a single window: its own speaker, and p = 0 under a target
    plain = D.Diarizer(scorer, threshold=0.0).cluster(emb)
    for target in (None, 1.0, 0.9995):
        diar = D.Diarizer(scorer, threshold=0.0, target_energy=target)
        got = diar.cluster(emb)
        assert diar.target_energy is None and diar.pca_report == {} and all(np.array_equal(got[k], plain[k]) and got[k].dtype == plain[k].dtype for k in plain)
    # prepare_pca with such a target, or for a recording without a PCA, hands back prepare's rows bit for bit and no model
    for target, keys in ((1.0, list(emb)), (0.9995, list(emb)), (0.5, ["one"])):
        for k, (rows, model) in zip(keys, scorer.prepare_pca([emb[k] for k in keys], target)):
            assert model is None and torch.equal(rows, scorer.prepare(emb[k])), (target, k)
    diar = D.Diarizer(scorer, threshold=0.0, target_energy=0.5)
    got = diar.cluster(emb)
    assert diar.pca_report["one"] == 0 and got["one"].tolist() == [0] and all(v > 0 for k, v in diar.pca_report.items() if k != "one")
    # the scorers that have no PLDA model to project are refused by name
    from tf_kaldi_speaker_amd.misc import scoring as S
    with pytest.raises(ValueError, match="Diarizer: target_energy .* needs a BackendScorer in the plda mode, not CosineScorer"):
        D.Diarizer(S.CosineScorer(DEV), threshold=0.0, target_energy=0.9)
    lda = B.BackendScorer(backend, "lda_cos", DEV)
    with pytest.raises(ValueError, match="needs a BackendScorer in the plda mode, not BackendScorer in the lda_cos mode"):
        D.Diarizer(lda, threshold=0.0, target_energy=0.9)
    with pytest.raises(ValueError, match="BackendScorer.prepare_pca: the per-recording PCA needs the plda mode"):
        lda.prepare_pca([emb["recA"]], 0.9)
    with pytest.raises(ValueError, match=r"BackendScorer.prepare_pca: target_energy must lie in \(0, 1\]"):
        scorer.prepare_pca([emb["recA"]], 1.2)
    with pytest.raises(ValueError, match="BackendScorer.dense: a per-recording model needs the plda mode"):
        lda.dense(lda.prepare(emb["recA"]), model=(2, None, None, None))


def test_vbx_behind_the_pca_runs_in_the_unreduced_space():
    from tf_kaldi_speaker_amd.misc import diarization as D
    scorer, recos = TV._scorer()
    emb = {k: x for k, (x, _) in recos.items()}
    truth = {k: TD._first_appearance(who) for k, (_, who) in recos.items()}
    # a threshold that over-splits under the recordings' own models: above three tenths of every recording's same-speaker scores
    cut = -np.inf
    for (x, who), (prepared, model) in zip(recos.values(), scorer.prepare_pca(list(emb.values()), 0.9)):
        s = scorer.dense(prepared, model=model).cpu().numpy()
        same = np.equal.outer(who, who) & np.triu(np.ones((len(who), len(who)), bool), 1)
        cut = max(cut, float(np.quantile(s[same], 0.3)))
    diar = D.Diarizer(scorer, threshold=cut, vbx=D.VbxOptions(), target_energy=0.9)
    got = diar.cluster(emb)
    plain = D.Diarizer(scorer, threshold=cut, target_energy=0.9).cluster(emb)
    assert list(got) == list(emb) and list(diar.vbx_report) == list(emb) == list(diar.pca_report)
    for k, (before, after, iters, elbo) in diar.vbx_report.items():
        assert before == min(int(plain[k].max()) + 1, 32) and 1 <= after <= before and 1 <= iters <= 20 and np.isfinite(elbo)
        assert got[k].tolist() == TD._first_appearance(got[k]) and int(got[k].max()) + 1 == after and 0 < diar.pca_report[k] <= scorer.dim
    print("VBx behind the PCA: speakers before / after %s, the true partition found: %s"
          % ({k: v[:2] for k, v in diar.vbx_report.items()}, {k: got[k].tolist() == truth[k] for k in got}))


def test_driver_with_target_energy(tmp_path):
    from tf_kaldi_speaker_amd.dataset import kaldi_io
    from tf_kaldi_speaker_amd.misc import backend as B
    from tf_kaldi_speaker_amd.misc import diarization as D
    tmp = str(tmp_path)
    model = os.path.join(tmp, "exp")
    TD._model(model)
    rs = np.random.RandomState(23)
    feats = {}
    for reco, frames in (("rec1", 1800), ("rec2", 1300)):
        tilt = np.where(np.arange(frames)[:, None] < frames // 2, np.linspace(-2, 2, 30)[None, :], np.linspace(2, -2, 30)[None, :])
        feats[reco] = (rs.randn(frames, 30) + tilt + 3.0).astype(np.float32)
    with open(os.path.join(tmp, "feats.ark"), "wb") as f:
        for reco, m in feats.items():
            kaldi_io.write_mat(f, m, key=reco)
    with open(os.path.join(tmp, "reco2num_spk"), "w") as f:
        f.write("rec1 2\nrec2 2\n")
    windows = {reco: D.subsegments(0, m.shape[0], 150, 75, 50) for reco, m in feats.items()}
    tail = [model, "ark:" + os.path.join(tmp, "feats.ark")]
    emb0 = os.path.join(tmp, "emb0.ark")
    TD._diarize(["--threshold", "0.5", "--write-embeddings", emb0] + tail + [os.path.join(tmp, "cos.rttm")])
    bdir = os.path.join(tmp, "backend")
    be = TV._backend_dir(bdir, emb0)
    scorer = B.BackendScorer(be, "plda", DEV)
    common = ["--backend", bdir, "--scoring", "plda", "--reco2num-spk", os.path.join(tmp, "reco2num_spk")]
    # without the option: today's bytes and no word of a PCA
    rttm0 = os.path.join(tmp, "plain.rttm")
    stderr = TD._diarize(common + tail + [rttm0])
    assert "PCA" not in stderr
    # with it: the RTTM the planner's windows and the restatement's scores and clustering give
    emb, rttm = os.path.join(tmp, "pca.ark"), os.path.join(tmp, "pca.rttm")
    stderr = TD._diarize(common + ["--target-energy", "0.5", "--write-embeddings", emb] + tail + [rttm])
    vecs = dict(kaldi_io.read_vec_flt_ark(emb))
    lines = []
    for reco, ws in windows.items():
        x = np.stack([vecs["%s-%07d-%07d" % (reco, s, e)] for s, e in ws])
        ref, p = _reference_scores(scorer, x, 0.5)
        prepared, own = scorer.prepare_pca([x], 0.5)[0]
        delta = float(np.abs(scorer.dense(prepared, model=own).cpu().numpy() - ref).max())
        labels = A.cluster(ref, target=2, dtype=np.float64)[0]
        print("driver, recording %s: p = %d, device - restatement %.3e, smallest merge margin %.3e, partition gap %.3e"
              % (reco, p, delta, _margin(ref, target=2), _partition_gap(ref, labels)))
        assert _decided(ref, labels, delta, target=2)
        assert "Recording %s: per-recording PCA: %d of 6 dimensions kept." % (reco, p) in stderr
        for a, b, l in D.rttm_turns(ws, labels):
            lines.append("SPEAKER %s 0 %.3f %.3f <NA> <NA> %d <NA> <NA>" % (reco, a * 0.01, (b - a) * 0.01, l + 1))
    assert open(rttm).read() == "".join(ln + "\n" for ln in lines) and lines
    # a target within 0.001 of 1: no PCA at all, the bytes of the run without the option
    rttm1 = os.path.join(tmp, "one.rttm")
    stderr = TD._diarize(common + ["--target-energy", "1"] + tail + [rttm1])
    assert open(rttm1).read() == open(rttm0).read() and "PCA" not in stderr
    # refusals, by their messages
    for args, what in ((["--threshold", "0.1", "--target-energy", "0.9"], "--target-energy needs --scoring plda"),
                       (["--threshold", "0.1", "--target-energy", "0.9", "--backend", bdir, "--scoring", "lda_cos"], "--target-energy needs --scoring plda"),
                       (common + ["--target-energy", "0"], "--target-energy must lie in (0, 1] (got 0)"),
                       (common + ["--target-energy", "1.5"], "--target-energy must lie in (0, 1] (got 1.5)")):
        assert what in TD._diarize(args + tail + [os.path.join(tmp, "no.rttm")], ok=False)
