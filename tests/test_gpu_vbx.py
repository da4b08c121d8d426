"""xv_vbx (csrc/xv_vbx.hip) at op level on a real MI355X against the NumPy restatement of tests/vbx_ref.py on the same float32 inputs.
One iteration: gamma, pi and the ELBO at most 8 x as far from the float64 restatement as its float32 evaluation is (never tighter than
16 * 2^-24 on gamma and pi, than 16 * 2^-24 (|tll| + |second term|) on the ELBO).  Many iterations: tolerances mean nothing across
iterations (float32 and float64 trajectories part while duplicate speakers merge), so the tests assert bit-equalities - k iterations in
one call == k chained calls, call == call, alone == third of four -, the stop rule on the kernel's own ELBO list, and after 20 iterations the
float64 restatement's labels on inputs whose every row has a gap of 0.5 between its two largest responsibilities (tests/test_vbx_ref.py
checks that condition without a GPU).  Every refusal is by name.  $XV_BOUNDS_OUT names a file that receives the largest error /
allowance ratios (profiles/vbx_bounds.txt)."""
import atexit
import os

import numpy as np
import pytest

from tests import vbx_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U16 = 16 * 2.0 ** -24
WORST = {}


def note(name, ratio):
    WORST[name] = max(WORST.get(name, 0.0), float(ratio))


@atexit.register
def _write_ledger():
    path = os.environ.get("XV_BOUNDS_OUT")
    if path and WORST:
        with open(path, "a") as f:
            f.write("# xv_vbx, one iteration: largest |kernel - float64| / max(8 |float32 NumPy - float64|, floor) over tests/test_gpu_vbx.py\n")
            for name in sorted(WORST):
                f.write("%-64s %.4f\n" % (name, WORST[name]))


def run(cases, params, max_iters, epsilon, extra_pitch=0, gap=0, state=None):
    """ops.vbx over the recordings `cases` (dicts of vbx_ref.make_case) packed at pitch D + extra_pitch with `gap` floats of NaN between
    them; state: [(gamma, pi)] to start from instead of the cases' own.  -> [(gamma [T, S], pi [S], elbo [max_iters], n_iters, labels)]."""
    import torch
    from tf_kaldi_speaker_amd import ops
    fa, fb, lp = params
    d = cases[0]["x"].shape[1]
    ld = d + extra_pitch
    t = np.asarray([c["x"].shape[0] for c in cases], np.int64)
    s = np.asarray([c["pi"].shape[0] for c in cases], np.int64)
    offsets = np.concatenate([[0], np.cumsum(t * ld + gap)])[:-1] + gap
    host = np.full(int(offsets[-1] + t[-1] * ld + gap), np.nan, np.float32)
    for c, off, rows in zip(cases, offsets, t):
        host[off:off + rows * ld].reshape(rows, ld)[:, :d] = c["x"]
    state = state or [(c["gamma"], c["pi"]) for c in cases]
    x = torch.from_numpy(host).to(DEV)
    phi = torch.from_numpy(np.array(cases[0]["phi"], np.float32)).to(DEV)
    gamma = torch.from_numpy(np.concatenate([np.asarray(g, np.float32).ravel() for g, _ in state])).to(DEV)
    pi = torch.from_numpy(np.concatenate([np.asarray(p, np.float32) for _, p in state])).to(DEV)
    before = (x.clone(), phi.clone(), gamma.clone(), pi.clone())
    g_out, p_out, elbo, n_iters, labels = ops.vbx(x, offsets, t, d, phi, gamma, pi, s, ld=np.full(len(cases), ld), loop_prob=lp, fa=fa, fb=fb,
                                                  max_iters=max_iters, epsilon=epsilon)
    torch.cuda.synchronize()
    for a, b in zip(before, (x, phi, gamma, pi)):      # X, Phi and the start are untouched (NaN padding included)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    g_out, p_out, elbo, n_iters, labels = (a.cpu().numpy() for a in (g_out, p_out, elbo, n_iters, labels))
    out, at, ats, atp = [], 0, 0, 0
    for j in range(len(cases)):
        out.append((g_out[ats:ats + t[j] * s[j]].reshape(t[j], s[j]), p_out[atp:atp + s[j]], elbo[j], int(n_iters[j]), labels[at:at + t[j]]))
        at, ats, atp = at + t[j], ats + t[j] * s[j], atp + s[j]
    return out


def check_one_iteration(name, got, shape, params):
    g, p, elbo, n_iters, labels = got
    g6, p6, e6, tll, second = R.one_iteration(shape, params, np.float64)
    g3, p3, e3 = R.one_iteration(shape, params, np.float32)[:3]
    assert n_iters == 1 and np.isfinite(g).all() and np.isfinite(p).all() and np.isnan(elbo[1:]).all()
    ratios = (np.abs(g - g6).max() / max(8 * np.abs(g3 - g6).max(), U16), np.abs(p - p6).max() / max(8 * np.abs(p3 - p6).max(), U16),
              abs(elbo[0] - e6) / max(8 * abs(e3 - e6), U16 * (abs(tll) + abs(second))))
    print("%s: error / allowance gamma %.4f pi %.4f ELBO %.4f (errors %.3e %.3e %.3e; float32 NumPy %.3e %.3e %.3e)"
          % (name, *ratios, np.abs(g - g6).max(), np.abs(p - p6).max(), abs(elbo[0] - e6), np.abs(g3 - g6).max(), np.abs(p3 - p6).max(), abs(e3 - e6)))
    for what, ratio in zip(("gamma", "pi", "elbo"), ratios):
        note("%s %s" % (what, name), ratio)
    assert max(ratios) <= 1.0, (name, ratios)
    assert np.array_equal(labels, np.argmax(g, axis=1))      # lowest s on a tie: argmax's rule


@pytest.mark.parametrize("params", R.PARAMS, ids=lambda p: "fa%g-fb%g-loop%g" % p)
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_one_iteration_against_float64(shape, params):
    got = run([R.case(shape)], params, 1, -np.inf, extra_pitch=0 if shape[1] % 8 else 3, gap=0 if shape[0] % 2 else 5)
    check_one_iteration("%dx%dx%d/%g,%g,%g" % (shape + params), got[0], shape, params)


def test_a_batch_of_mixed_lengths():
    """T = 1, 65, 257 and 2 in one call: recordings of another D cannot share a call (one model), so the rows of the shared cases are cut
    to 8 dimensions here and the references computed for these inputs."""
    params = R.PARAMS[0]
    cases = []
    for shape in ((1, 8, 1), (65, 8, 4), (257, 8, 7), (2, 8, 2)):
        c = R.make_case(*shape, seed=1)
        cases.append(c)
    got = run(cases, params, 1, -np.inf, extra_pitch=1, gap=3)
    fa, fb, lp = params
    for c, (g, p, elbo, n_iters, labels) in zip(cases, got):
        g6, p6, e6, tll, second = R.iteration_scaled(c["x"], c["phi"], c["gamma"], c["pi"], lp, fa, fb, np.float64)
        g3, p3, e3 = R.iteration_scaled(c["x"], c["phi"], c["gamma"], c["pi"], lp, fa, fb, np.float32)[:3]
        assert n_iters == 1
        assert np.abs(g - g6).max() <= max(8 * np.abs(g3 - g6).max(), U16) and np.abs(p - p6).max() <= max(8 * np.abs(p3 - p6).max(), U16)
        assert abs(elbo[0] - e6) <= max(8 * abs(e3 - e6), U16 * (abs(tll) + abs(second)))
    # ... and each of them alone gives the bits it gave in the batch
    for c, batch in zip(cases, got):
        alone = run([c], params, 1, -np.inf)[0]
        assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(alone, batch))


@pytest.mark.parametrize("params", R.PARAMS, ids=lambda p: "fa%g-fb%g-loop%g" % p)
@pytest.mark.parametrize("shape", [(2, 4, 2), (65, 8, 4), (257, 36, 7), (600, 128, 10)], ids=lambda s: "%dx%dx%d" % s)
def test_iterations_chain_bit_for_bit(shape, params):
    k = 5
    c = R.case(shape)
    whole = run([c], params, k, -np.inf)[0]
    assert whole[3] == k and np.isfinite(whole[2]).all()
    state, elbos = [(c["gamma"], c["pi"])], []
    for _ in range(k):
        g, p, elbo, n_iters, labels = run([c], params, 1, -np.inf, state=state)[0]
        assert n_iters == 1
        state, elbos = [(g, p)], elbos + [elbo[0]]
    assert np.array_equal(whole[0], g) and np.array_equal(whole[1], p) and np.array_equal(whole[2], np.asarray(elbos)) and np.array_equal(whole[4], labels)
    again = run([c], params, k, -np.inf)[0]      # two calls: the same bits
    assert all(np.array_equal(a, b) for a, b in zip(whole, again))
    others = [R.case(s) for s in R.SHAPES if s[1] == shape[1] and s != shape] or [R.make_case(33, shape[1], 3, 5)]
    four = run([others[0], R.make_case(9, shape[1], 2, 6), c, others[-1]], params, k, -np.inf, extra_pitch=2)      # alone == the third of four
    assert all(np.array_equal(a, b) for a, b in zip(whole, four[2]))


def test_the_cap_chains_and_repeats():
    shape, params = (2048, 256, 32), R.PARAMS[1]
    c = R.case(shape)
    whole = run([c], params, 2, -np.inf)[0]
    g, p, e0 = run([c], params, 1, -np.inf)[0][:3]
    g, p, e1 = run([c], params, 1, -np.inf, state=[(g, p)])[0][:3]
    assert np.array_equal(whole[0], g) and np.array_equal(whole[1], p) and whole[2].tolist() == [e0[0], e1[0]]


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_twenty_iterations_give_the_float64_labels(shape):
    seed = R.gap_checked_seed(shape)
    c = R.case(shape, seed)
    g64, labels64, _ = R.converged(shape, seed)
    assert R.row_gap(g64) >= 0.5      # the condition on the inputs; no row is left out below
    g, p, elbo, n_iters, labels = run([c], R.PARAMS[0], 20, -np.inf)[0]
    assert n_iters == 20 and np.isfinite(elbo).all()
    assert np.array_equal(labels, labels64)
    assert np.array_equal(R.first_appearance(labels), R.first_appearance(c["who"]))      # the true partition


def test_stop_rule_on_the_kernels_own_elbo():
    shape, params = (65, 8, 4), R.PARAMS[0]
    c = R.case(shape)
    full = run([c], params, 20, -np.inf)[0]
    gains = np.diff(full[2])
    candidates = [i for i in range(2, 12) if gains[i] < gains[:i].min() and gains[i] > 0]
    assert candidates, gains
    i = candidates[0]
    eps = 0.5 * (gains[i] + gains[:i].min())      # the gains before iteration i + 1 are above eps, its own is below
    g, p, elbo, n_iters, labels = run([c], params, 20, eps)[0]
    first = 1 + int(np.argmax(np.diff(elbo[:n_iters]) < eps))      # the first iteration (index >= 1) whose gain is below eps ...
    assert n_iters == first + 1 == i + 2 < 20                       # ... is the last one run
    assert np.array_equal(elbo[:n_iters], full[2][:n_iters]) and np.isnan(elbo[n_iters:]).all()      # the entries beyond it are untouched
    assert np.array_equal(g, run([c], params, n_iters, -np.inf)[0][0])
    # a batch stops per recording; +inf stops after the second iteration, never after the first
    two = run([c, R.make_case(40, 8, 3, 2)], params, 7, np.inf)
    assert [r[3] for r in two] == [2, 2] and all(np.isnan(r[2][2:]).all() and np.isfinite(r[2][:2]).all() for r in two)
    assert run([c], params, 1, np.inf)[0][3] == 1


def test_a_dead_speaker_stays_dead_without_nan():
    c = dict(R.case((65, 8, 4)))
    c["pi"] = np.array([0.5, 0.0, 0.25, 0.25], np.float32)
    x = c["x"].copy()
    x[7] *= 40.0      # a row far from every live model, where the dead speaker's flat model scores best by far
    c["x"] = x
    g, p, elbo, n_iters, labels = run([c], R.PARAMS[0], 3, -np.inf)[0]
    assert n_iters == 3 and np.isfinite(g).all() and np.isfinite(p).all() and np.isfinite(elbo).all()
    assert (g[:, 1] == 0).all() and p[1] == 0 and abs(float(p.sum()) - 1) < 1e-6 and (labels != 1).all()
    fa, fb, lp = R.PARAMS[0]
    g6, p6 = c["gamma"], c["pi"]
    g6, p6, e6 = R.iteration_scaled(c["x"], c["phi"], g6, p6, lp, fa, fb, np.float64)[:3]
    one = run([c], R.PARAMS[0], 1, -np.inf)[0]
    assert np.abs(one[0] - g6).max() < 1e-4 and abs(one[2][0] - e6) < 1e-5 * abs(e6)


def test_refusals_by_name():
    import torch
    from tf_kaldi_speaker_amd import ops
    from tf_kaldi_speaker_amd.misc import backend as B
    assert (ops.VBX_MAX_SPEAKERS, ops.VBX_MAX_DIM, ops.AHC_MAX_N) == (32, 256, 2048)
    z = lambda n: torch.zeros(n, dtype=torch.float32, device=DEV)

    def call(t=3, d=4, s=2, ld=None, off=0, x_floats=None, **kw):
        ld_ = d if ld is None else ld
        return ops.vbx(z(x_floats if x_floats is not None else max(t, 1) * max(ld_, d, 1)), [off], [t], d, z(max(d, 1)), z(max(t * s, 1)), z(max(s, 1)), [s],
                       ld=None if ld is None else [ld], **kw)

    for kw, exc, what in ((dict(t=0), ValueError, "vbx: recording 0 has no row"),
                          (dict(t=2049), ValueError, "vbx: recording 0 has 2049 rows, the cap is 2048"),
                          (dict(s=0), ValueError, "vbx: recording 0 has no speaker"),
                          (dict(s=33), ValueError, "vbx: recording 0 has 33 speakers, the cap is 32"),
                          (dict(d=0), ValueError, r"vbx: d must lie in 1 \.\. 256 \(got 0\)"),
                          (dict(d=257), ValueError, r"vbx: d must lie in 1 \.\. 256 \(got 257\)"),
                          (dict(max_iters=0), ValueError, r"vbx: max_iters must lie in 1 \.\. 64 \(got 0\)"),
                          (dict(max_iters=65), ValueError, r"vbx: max_iters must lie in 1 \.\. 64 \(got 65\)"),
                          (dict(loop_prob=0.0), ValueError, "vbx: loop_prob must lie strictly between 0 and 1"),
                          (dict(loop_prob=1.0), ValueError, "vbx: loop_prob must lie strictly between 0 and 1"),
                          (dict(loop_prob=1.0 - 1e-12), ValueError, "vbx: loop_prob must lie strictly between 0 and 1 as a float32"),
                          (dict(fa=0.0), ValueError, "vbx: fa and fb must be positive"),
                          (dict(fb=-1.0), ValueError, "vbx: fa and fb must be positive"),
                          (dict(epsilon=float("nan")), ValueError, "vbx: epsilon is not a number"),
                          (dict(ld=3), ValueError, "vbx: recording 0: the pitch 3 is below the 4 dimensions"),
                          (dict(off=1), IndexError, "vbx: a recording's rows lie outside the 12 floats of x"),
                          (dict(off=-1, x_floats=40), IndexError, "vbx: a recording's rows lie outside the 40 floats of x"),
                          (dict(ld=6, x_floats=15), IndexError, "vbx: a recording's rows lie outside the 15 floats of x")):
        with pytest.raises(exc, match=what):
            call(**kw)
    with pytest.raises(ValueError, match=r"vbx: gamma \(sum of t \* s\) must be 6 contiguous float32 values"):
        ops.vbx(z(12), [0], [3], 4, z(4), z(5), z(2), [2])
    with pytest.raises(ValueError, match=r"vbx: pi \(sum of s\) must be 2 contiguous float32 values"):
        ops.vbx(z(12), [0], [3], 4, z(4), z(6), z(3), [2])
    with pytest.raises(ValueError, match="vbx: s must be a 1-D integer array of 1"):
        ops.vbx(z(12), [0], [3], 4, z(4), z(6), z(2), [2, 2])
    # the last row may end with the buffer: ld = 6 needs 2 * 6 + 4 = 16 floats
    assert ops.vbx(z(16), [0], [3], 4, torch.ones(4, device=DEV), torch.full((6,), 0.5, device=DEV), torch.full((2,), 0.5, device=DEV), [2], ld=[6],
                   max_iters=1)[3].tolist() == [1]
    # a back end without PLDA
    rs = np.random.RandomState(0)
    lda_only = B.Backend(rs.randn(6).astype(np.float32), rs.randn(3, 7).astype(np.float32), None)
    with pytest.raises(ValueError, match="BackendScorer.plda_space: needs a PLDA model and the plda mode"):
        B.BackendScorer(lda_only, "lda_cos", DEV).plda_space(rs.randn(5, 6).astype(np.float32))
