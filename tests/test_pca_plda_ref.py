"""CPU checks of the per-recording PCA of PLDA scoring: the fp64 restatement tests/pca_plda_ref.py against the properties that define it,
the decision-gap conditions of every case the GPU tests use, and the host layers' arguments (misc/backend.py, misc/diarization.py,
diar_ops.py) that are refused before any launch."""
import numpy as np
import pytest

from tests import pca_plda_ref as P

ALL = [(d, n, t) for d, n, targets in P.SHAPES for t in targets] + [P.BIG]


@pytest.mark.parametrize("d,n,target", [s for s in ALL if s[0] <= 130])
def test_projected_model_is_diagonalised(d, n, target):
    c = P.case(d, n)
    m = P.estimate(c["x"], c["w"], c["b"], c["mu"], target)
    p = m["p"]
    assert m["q"].shape == (p, d) and np.abs(m["q"] @ m["q"].T - np.eye(p)).max() < 1e-12
    assert np.abs(m["tp"] @ m["wp"] @ m["tp"].T - np.eye(p)).max() < 1e-11
    assert np.abs(m["tp"] @ m["bp"] @ m["tp"].T - np.diag(m["psi"])).max() < 1e-11 * max(1.0, m["psi"][0])
    assert np.all(np.diff(m["psi"]) <= 0) and m["psi"][-1] >= 0.0
    # the map takes a unit-length row to what the recipe's sqrt(D)-length row would give: A W A^T / D = I
    assert np.abs(m["a"] @ c["w"] @ m["a"].T / d - np.eye(p)).max() < 1e-11
    assert np.allclose(m["offset"], -(m["a"] @ c["mu"]) / np.sqrt(d), rtol=0, atol=1e-12)


def test_scores_do_not_depend_on_the_basis_of_the_subspace():
    """Q -> R Q for a random orthogonal R: W', B' and T' change, the scores do not - which is why the GPU test compares scores and not
    eigenvectors.  Scores of size 30 agree to 3e-14 here; asserted at 1e-11 of the largest."""
    c = P.case(36, 40)
    want = P.scores(c["x"], c["w"], c["b"], c["mu"], 0.9)
    p = P.estimate(c["x"], c["w"], c["b"], c["mu"], 0.9)["p"]
    r = np.linalg.qr(np.random.RandomState(4).randn(p, p))[0]
    got = P.scores(c["x"], c["w"], c["b"], c["mu"], 0.9, basis=r)
    print("basis invariance: %.3e of %.3e" % (np.abs(got - want).max(), np.abs(want).max()))
    assert np.abs(got - want).max() <= 1e-11 * np.abs(want).max()


def test_energy_rule_keeps_one_row_more_than_the_energy_needs():
    s = np.array([4.0, 3.0, 2.0, 1.0])
    assert P.energy_dim(s, 0.3) == 2       # the first eigenvalue holds 0.4 > 0.3: k = 1, p = 2
    assert P.energy_dim(s, 0.5) == 3       # 0.4, then 0.7 > 0.5: k = 2, p = 3
    assert P.energy_dim(s, 0.4) == 3       # 0.4 <= 0.4 goes on: "more than", not "at least"
    assert P.energy_dim(s, 0.95) == 4 and P.energy_dim(s, 1.0) == 4      # capped at D
    for d, n, target in ALL[:8]:
        c = P.case(d, n)
        m = P.estimate(c["x"], c["w"], c["b"], c["mu"], target)
        share = np.cumsum(m["s"]) / m["s"].sum()
        k = int(np.argmax(share > target)) + 1
        assert m["p"] == min(k + 1, d)


def test_a_single_row_and_a_zero_covariance_give_no_model():
    c = P.case(5, 3)
    assert P.estimate(c["x"][:1], c["w"], c["b"], c["mu"], 0.5)["p"] == 0
    assert P.estimate(np.repeat(c["x"][:1], 4, axis=0), c["w"], c["b"], c["mu"], 0.5)["p"] == 0      # four equal rows: C = 0 exactly
    assert P.scores(c["x"][:1], c["w"], c["b"], c["mu"], 0.5) is None


@pytest.mark.parametrize("d,n,target", ALL)
def test_every_case_meets_the_decision_gap_conditions(d, n, target):
    """|E_k / E - target| >= 1e-9 for every k, (s_p - s_{p+1}) >= 1e-6 s_1 when p < D, p <= rank C: on the reference alone."""
    x = P.case(d, n)["x"]
    egap, sgap, p, rank = P.decision_gaps(x, target)
    print("D=%d n=%d target=%g: p=%d rank=%d energy gap %.2e eigenvalue gap %.2e s_1" % (d, n, target, p, rank, egap, sgap))
    assert egap >= 1e-9 and sgap >= 1e-6 and p <= rank and P.qualifies(x, target)
    assert np.abs(np.linalg.norm(x.astype(np.float64), axis=1) - 1.0).max() < 1e-6


def test_the_conditions_refuse_what_they_should():
    x = P.recording(0, 5, 3)
    assert not P.qualifies(x, 0.9999)                                  # p = 3 above the rank of 2
    s = P.estimate(x, np.eye(5), np.eye(5), np.zeros(5), 0.5)["s"]
    assert not P.qualifies(x, float(s[0] / s.sum()))                   # the target on an energy step


def test_host_layers():
    from tf_kaldi_speaker_amd.misc import backend as B
    from tf_kaldi_speaker_amd.misc import diarization as D
    plda = P.model(3, 7)
    w, b, mu = B.plda_covariances(plda)
    rw, rb = P.covariances(plda)
    assert np.array_equal(w, w.T) and np.array_equal(b, b.T) and np.allclose(w, rw, rtol=0, atol=1e-14) and np.allclose(b, rb, rtol=0, atol=1e-13)
    t = plda["transform"]
    assert np.abs(t @ w @ t.T - np.eye(7)).max() < 1e-12 and np.abs(t @ b @ t.T - np.diag(plda["psi"])).max() < 1e-11 and np.array_equal(mu, plda["mean"])
    assert B.check_target_energy(None, "x") is None and B.check_target_energy(1, "x") == 1.0
    for bad in (0.0, -0.5, 1.0001, float("nan")):
        with pytest.raises(ValueError, match=r"x: target_energy must lie in \(0, 1\]"):
            B.check_target_energy(bad, "x")

    class NoPlda(object):
        torch = ops = None
    with pytest.raises(ValueError, match="Diarizer: target_energy .* needs a BackendScorer in the plda mode, not NoPlda"):
        D.Diarizer(NoPlda(), threshold=0.0, target_energy=0.9)

    class Plda(object):
        torch = ops = None
        mode = "plda"

        def prepare_pca(self, matrices, target):
            raise AssertionError("not called here")
    for bad in (0.0, 1.5, -1.0):
        with pytest.raises(ValueError, match=r"Diarizer: target_energy must lie in \(0, 1\]"):
            D.Diarizer(Plda(), threshold=0.0, target_energy=bad)
    assert D.Diarizer(Plda(), threshold=0.0, target_energy=0.9).target_energy == 0.9
    assert D.Diarizer(Plda(), threshold=0.0, target_energy=0.9995).target_energy is None      # within 0.001 of 1: no PCA at all
    assert D.Diarizer(Plda(), threshold=0.0).target_energy is None
    Plda.mode = "lda_cos"
    with pytest.raises(ValueError, match="needs a BackendScorer in the plda mode, not Plda in the lda_cos mode"):
        D.Diarizer(Plda(), threshold=0.0, target_energy=0.9)


def test_entry_points_are_declared_and_refuse_by_name():
    """The C entry points check their host arguments before any launch: no GPU is touched by a refused call."""
    import ctypes as C
    from tf_kaldi_speaker_amd import _lib
    lib = _lib.load()
    assert "xv_backend_pca_plda" in _lib.SIGNATURES and "xv_backend_pca_plda_workspace_bytes" in _lib.SIGNATURES
    assert lib.xv_backend_pca_plda_workspace_bytes(3, 5) == 3 * 4 * 36 * 8 and lib.xv_backend_pca_plda_workspace_bytes(1, 256) == 4 * 65536 * 8
    assert lib.xv_backend_pca_plda_workspace_bytes(0, 5) == 0 and lib.xv_backend_pca_plda_workspace_bytes(1, 257) == 0
    p = C.c_void_p(4096)

    def call(b=1, d=4, max_n=3, target=0.5, ws=p, ws_bytes=1 << 20):
        return lib.xv_backend_pca_plda(None, p, 12, p, p, p, b, d, max_n, target, p, p, p, p, p, p, p, p, p, p, p, p, p, ws, ws_bytes)
    for kw, text in ((dict(b=0), "no recording in the call"), (dict(d=0), "d must lie in 1 .. 256 (got 0)"), (dict(d=257), "d must lie in 1 .. 256 (got 257)"),
                     (dict(max_n=0), "at least one row"), (dict(max_n=2049), "a recording of 2049 rows exceeds the cap of 2048"),
                     (dict(target=0.0), "target must lie in (0, 1] (got 0)"), (dict(target=1.5), "target must lie in (0, 1] (got 1.5)"),
                     (dict(target=float("nan")), "target must lie in (0, 1]"), (dict(ws=None), "workspace of"),
                     (dict(ws_bytes=4 * 16 * 8 - 1), "workspace of 511 bytes, 512 needed"), (dict(ws=C.c_void_p(4104)), "16-byte aligned")):
        assert call(**kw) != 0 and text in lib.xv_last_error().decode(), (kw, lib.xv_last_error())
