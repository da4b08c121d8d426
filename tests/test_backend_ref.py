"""The restatement of the LDA / PLDA back end (tests/backend_ref.py) and the host side of misc/backend.py, pinned by derivations that
share no code with either: the log-likelihood ratio from 2 x 2 Gaussians, the simultaneous-diagonalisation invariants of both estimators,
a planted model, the file round trips, the host plumbing and the refusals of the command line.  No GPU."""
import io
import logging
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from tests import backend_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "tf_kaldi_speaker_amd")


def _log_normal(x, cov):
    """log N(x; 0, cov) from the covariance itself."""
    x, cov = np.atleast_1d(x).astype(np.float64), np.atleast_2d(cov).astype(np.float64)
    return -0.5 * (len(x) * np.log(2 * np.pi) + np.log(np.linalg.det(cov)) + x @ np.linalg.solve(cov, x))


@pytest.mark.parametrize("n", [1, 3, 8])
def test_llr_from_first_principles(n):
    """Per dimension, the closed form equals log N([e; t]; 0, [[psi + 1/n, psi], [psi, psi + 1]]) - log N(e; 0, psi + 1/n) - log N(t; 0, psi + 1)."""
    rs = np.random.RandomState(n)
    d = 7
    psi = rs.uniform(0.05, 5.0, d)
    e, t = rs.randn(d) * 2, rs.randn(d) * 2
    want = 0.0
    for c in range(d):
        joint = np.array([[psi[c] + 1.0 / n, psi[c]], [psi[c], psi[c] + 1.0]])
        want += _log_normal([e[c], t[c]], joint) - _log_normal(e[c], psi[c] + 1.0 / n) - _log_normal(t[c], psi[c] + 1.0)
    got = R.llr(e, t, psi, n)
    assert abs(got - want) <= 1e-10 * abs(want)
    vec = R.llr_trials(e[None, :], t[None, :], [0], [0], psi, [n])[0]
    assert abs(vec - want) <= 1e-10 * abs(want)


def _planted_plda(seed, speakers=400, d=12):
    rs = np.random.RandomState(seed)
    rot = np.linalg.qr(rs.randn(d, d))[0]
    between = rot @ np.diag([4.0, 3.0, 2.0, 1.0] + [0.0] * (d - 4)) @ rot.T
    a = rs.randn(d, d)
    spd = a @ a.T / d + 0.5 * np.eye(d)
    lw = np.linalg.cholesky(spd)                                    # within = I rotated by a random SPD
    lb = rot @ np.diag(np.sqrt([4.0, 3.0, 2.0, 1.0] + [0.0] * (d - 4)))
    groups, rows, at = [], [], 0
    for n in rs.choice([1, 2, 5, 9], speakers):
        m = lb @ rs.randn(d) + 0.7
        rows.append(m[None, :] + rs.randn(n, d) @ lw.T)
        groups.append(list(range(at, at + n)))
        at += n
    return np.concatenate(rows), groups, between, spd


def _canon(transform):
    """Rows with their largest entry positive: an eigenvector's sign is not defined."""
    sign = np.sign(transform[np.arange(len(transform)), np.abs(transform).argmax(axis=1)])
    return transform * sign[:, None]


def test_plda_estimator_invariants_and_planted_model():
    from tf_kaldi_speaker_amd.misc import backend as B
    y, groups, _, _ = _planted_plda(1)
    s, means, counts = R.plda_stats(y, groups)
    ref = R.plda_em(s, means, counts)
    got = B.estimate_plda(y.T @ y, means, counts, num_em_iters=10)
    for m in (ref, got):
        t, w, b, psi = m["transform"], m["within"], m["between"], m["psi"]
        assert np.abs(t @ w @ t.T - np.eye(len(psi))).max() <= 1e-9
        assert np.abs(t @ b @ t.T - np.diag(psi)).max() <= 1e-9 * max(1.0, psi.max())
        assert np.all(np.diff(psi) <= 0) and np.all(psi >= 0)
        assert np.array_equal(m["offset"], -(t @ m["mean"]))
    # the grouped EM from fp64 statistics equals the straight per-speaker loop
    scale = max(1.0, np.abs(ref["transform"]).max())
    assert np.abs(got["psi"] - ref["psi"]).max() <= 1e-9 * max(1.0, ref["psi"].max())
    assert np.abs(got["within"] - ref["within"]).max() <= 1e-9 and np.abs(got["between"] - ref["between"]).max() <= 1e-9
    assert np.abs(got["mean"] - ref["mean"]).max() <= 1e-12
    assert np.abs(_canon(got["transform"]) - _canon(ref["transform"])).max() <= 1e-9 * scale
    # the planted between-class covariance has rank 4: four psi stand out
    assert ref["psi"][3] > 5 * ref["psi"][4]


def test_lda_invariants_on_a_planted_subspace():
    from tf_kaldi_speaker_amd.misc import backend as B
    rs = np.random.RandomState(2)
    d, dim = 24, 8
    basis = np.linalg.qr(rs.randn(d, d))[0][:, :dim] * np.linspace(6.0, 4.0, dim)[None, :]
    groups, rows, at = [], [], 0
    for n in rs.randint(2, 9, 200):
        rows.append((basis @ rs.randn(dim))[None, :] + rs.randn(n, d))
        groups.append(list(range(at, at + n)))
        at += n
    x = np.concatenate(rows)
    v = x - x.mean(axis=0)
    ref, l, floor_active, total, within = R.lda(v, groups, dim)
    assert not floor_active                                        # the floor is inactive on this data
    assert l[7] / l[8] > 10                                        # the cut sits in a wide eigenvalue gap
    means = np.asarray([v[g].mean(axis=0) for g in groups])
    counts = np.asarray([len(g) for g in groups])
    got, l_got = B.estimate_lda(v.T @ v, means, counts, dim)
    assert got.shape == (dim, d + 1) and np.abs(l_got - l).max() <= 1e-9 * l.max()
    for mat in (ref, got):
        a = mat[:, :d]
        assert np.abs(a @ within @ a.T - np.eye(dim)).max() <= 1e-9
        bt = a @ (total - within) @ a.T
        assert np.abs(bt - np.diag(np.diag(bt))).max() <= 1e-9 * np.abs(bt).max()
        assert np.all(np.diff(np.diag(bt)) <= 0)
        assert np.abs(mat[:, d] + a @ v.mean(axis=0)).max() <= 1e-9     # the offset column: -A mu', mu' about 0
    assert np.abs(_canon(got[:, :d]) - _canon(ref[:, :d])).max() <= 1e-9 * np.abs(ref).max()


def test_backend_round_trip_and_plda_bytes(tmp_path):
    from tf_kaldi_speaker_amd.dataset import kaldi_io
    from tf_kaldi_speaker_amd.misc import backend as B
    rs = np.random.RandomState(3)
    plda = dict(mean=rs.randn(3), transform=rs.randn(3, 3), psi=np.array([2.0, 1.0, 0.25]))
    be = B.Backend(rs.randn(5).astype(np.float32), rs.randn(3, 6).astype(np.float32), plda)
    be.save(str(tmp_path / "b"))
    assert sorted(os.listdir(tmp_path / "b")) == ["mean.vec", "plda", "transform.mat"]
    back = B.Backend.load(str(tmp_path / "b"))
    assert back.mean.tobytes() == be.mean.tobytes() and back.lda.tobytes() == be.lda.tobytes() and back.lda.shape == (3, 6)
    for k in ("mean", "transform", "psi"):
        assert back.plda[k].dtype == np.float64 and back.plda[k].tobytes() == plda[k].tobytes()
    assert (back.d, back.dim) == (5, 3)
    # the <Plda> object, byte by byte
    fixture = (b"\0B<Plda> " + b"DV \x04" + struct.pack("<i", 3) + plda["mean"].astype("<f8").tobytes()
               + b"DM \x04" + struct.pack("<i", 3) + b"\x04" + struct.pack("<i", 3) + plda["transform"].astype("<f8").tobytes()
               + b"DV \x04" + struct.pack("<i", 3) + plda["psi"].astype("<f8").tobytes() + b"</Plda> ")
    assert open(tmp_path / "b" / "plda", "rb").read() == fixture
    mean, transform, psi = kaldi_io.read_plda(io.BytesIO(fixture))
    assert np.array_equal(mean, plda["mean"]) and np.array_equal(transform, plda["transform"]) and np.array_equal(psi, plda["psi"])
    with pytest.raises(kaldi_io.BadInputFormat, match="does not start with"):
        kaldi_io.read_plda(io.BytesIO(b"\0B<Nnet> " + fixture[9:]))
    # an LDA-free, PLDA-free directory: the mean alone
    B.Backend(be.mean).save(str(tmp_path / "m"))
    only = B.Backend.load(str(tmp_path / "m"))
    assert only.lda is None and only.plda is None and only.dim == 5
    with pytest.raises(ValueError, match="no mean.vec"):
        B.Backend.load(str(tmp_path / "nothing"))
    with pytest.raises(ValueError, match="works on 3 dimensions"):
        B.Backend(be.mean, None, plda)


def test_spk2utt_and_group_index(tmp_path, caplog):
    from tf_kaldi_speaker_amd.misc import backend as B
    with open(tmp_path / "spk2utt", "w") as f:
        f.write("spkA u1 u2 u3\n\nspkB u4\nspkC u7 u8\nspkD u2 u5\n")
    s2u = B.read_spk2utt(str(tmp_path / "spk2utt"))
    assert s2u == [("spkA", ["u1", "u2", "u3"]), ("spkB", ["u4"]), ("spkC", ["u7", "u8"]), ("spkD", ["u2", "u5"])]
    for bad, what in (("spkA u1\nspkB\n", ":2: speaker spkB lists no utterance"), ("spkA u1\nspkA u2\n", ":2: speaker spkA is listed twice")):
        with open(tmp_path / "bad", "w") as f:
            f.write(bad)
        with pytest.raises(ValueError, match=what):
            B.read_spk2utt(str(tmp_path / "bad"))
    with caplog.at_level(logging.INFO, logger="tf_kaldi_speaker_amd"):
        gi = B.GroupIndex(["u5", "u4", "u2", "u1"], s2u)
    assert gi.names == ["spkA", "spkB", "spkD"] and gi.dropped == ["spkC"] and gi.skipped_utts == 3
    assert gi.offsets.tolist() == [0, 2, 3, 5] and gi.rows.tolist() == [3, 2, 1, 2, 0] and gi.counts.tolist() == [2, 1, 2]
    assert gi.offsets.dtype == np.int64 and gi.rows.dtype == np.int32
    text = caplog.text
    assert "Utterance u3 of speaker spkA: no vector, skip." in text and "Speaker spkC: no vector for any utterance, dropped." in text


def test_plda_coefficients_against_the_restatement():
    from tf_kaldi_speaker_amd.misc import backend as B
    psi = np.array([5.0, 2.5, 1.0, 0.3, 0.0])
    coef, g, k0 = B.plda_coefficients(psi, [1, 3, 8])
    a, iv, g_ref, k0_ref = R.coefficients(psi, [1, 3, 8])
    assert coef.shape == (3, 2, 8) and coef.dtype == np.float32 and g.shape == (8,) and k0.shape == (3,)
    assert np.array_equal(coef[:, 0, :5], a.astype(np.float32)) and np.array_equal(coef[:, 1, :5], iv.astype(np.float32))
    assert np.array_equal(g[:5], g_ref.astype(np.float32)) and np.allclose(k0, k0_ref, rtol=1e-7, atol=0)
    assert np.all(coef[:, :, 5:] == 0) and np.all(g[5:] == 0)
    # the tables reproduce the closed form
    rs = np.random.RandomState(0)
    e, t = rs.randn(4, 5), rs.randn(6, 5)
    ei, ti, n = np.array([0, 1, 2, 3, 3]), np.array([5, 0, 2, 2, 1]), np.array([1, 8, 3, 8])
    got, _, _ = R.trials_from_tables(e, t, ei, ti, np.searchsorted([1, 3, 8], n), coef, g, k0, 5)
    want = R.llr_trials(e, t, ei, ti, psi, n)
    assert np.abs(got - want).max() <= 1e-5
    with pytest.raises(ValueError, match="must be positive"):
        B.plda_coefficients(psi, [0])


def _score(args):
    env = dict(os.environ, TF_KALDI_ROOT=PKG, PYTHONPATH=PKG)
    return subprocess.run([sys.executable, os.path.join(PKG, "nnet", "lib", "score.py")] + args + ["trials", "ark:e.ark", "ark:t.ark", "out"], env=env,
                          capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("args,what", [
    (["--backend", "dir", "--scoring", "plda", "--cohort", "ark:c.ark"], "--cohort with --scoring plda is not supported"),
    (["--backend", "dir", "--scoring", "lda_cos", "--center-on", "ark:c.ark"], "--backend and --center-on exclude each other"),
    (["--scoring", "plda"], "--scoring plda needs --backend DIR"),
    (["--scoring", "lda_cos"], "--scoring lda_cos needs --backend DIR"),
])
def test_cli_refusals_by_name(args, what):
    """Refused before any file is opened or the GPU is touched (the files named here do not exist)."""
    r = _score(args)
    assert r.returncode != 0 and what in r.stderr, r.stderr[-500:]
