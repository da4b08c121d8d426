"""NumPy restatement of the VB-HMM clustering of x-vectors (VBx) that xv_vbx runs (include/xvector_hip.h states the arithmetic), twice
over: the log-domain form exactly as the operation is defined, float64 only, and the per-frame scaled form the kernel uses, with a dtype
argument (float32: the rounding the kernel is allowed; float64: the checker of the GPU tests).  Also the generator the GPU tests share,
so that its conditioning can be checked without a GPU (tests/test_vbx_ref.py).  VBx as recalled from BUT's VB_diarization.py: nothing
here is compared with a run of that code."""
import numpy as np

LOG_2PI = float(np.log(2.0 * np.pi))


def _lse(a, axis):
    """log sum exp along axis; a slice of -inf only gives -inf (a dead speaker), no NaN."""
    m = np.max(a, axis=axis, keepdims=True)
    m = np.where(np.isfinite(m), m, 0.0)
    with np.errstate(divide="ignore"):
        return np.log(np.sum(np.exp(a - m), axis=axis)) + np.squeeze(m, axis=axis)


def speaker_models(rho, phi, gamma, fa, fb):
    """Steps 1 and 2 without G: (scores' [T, S] = fa (rho alpha^T - 0.5 sum_d (invL + alpha^2) Phi_d), the ELBO's second term in double)."""
    dt = rho.dtype
    c = dt.type(fa) / dt.type(fb)
    n = gamma.sum(axis=0)
    inv_l = dt.type(1) / (dt.type(1) + c * n[:, None] * phi[None, :])
    alpha = c * inv_l * (gamma.T @ rho)
    scores = dt.type(fa) * (rho @ alpha.T - dt.type(0.5) * ((inv_l + alpha * alpha) * phi[None, :]).sum(axis=1)[None, :])
    il, al = inv_l.astype(np.float64), alpha.astype(np.float64)
    second = 0.5 * float(fb) * float(np.sum(np.log(il) - il - al * al + 1.0))
    return scores, second


def frame_terms(x, fa):
    """fa sum_t G_t in double, G_t = -0.5 (sum_d X_td^2 + D ln 2 pi)."""
    x64 = x.astype(np.float64)
    return float(fa) * float(np.sum(-0.5 * ((x64 * x64).sum(axis=1) + x.shape[1] * LOG_2PI)))


def iteration_log(x, phi, gamma, pi, loop_prob, fa, fb):
    """One iteration in the log domain, float64, as the operation is defined.  -> (gamma, pi, ELBO, tll, second term)."""
    x, phi, gamma, pi = (np.asarray(a, np.float64) for a in (x, phi, gamma, pi))
    t_rows, d = x.shape
    rho = x * np.sqrt(phi)[None, :]
    g = -0.5 * ((x * x).sum(axis=1) + d * LOG_2PI)
    scores, second = speaker_models(rho, phi, gamma, fa, fb)
    logp = scores + fa * g[:, None]
    s = pi.shape[0]
    with np.errstate(divide="ignore"):
        ltr = np.log(loop_prob * np.eye(s) + (1.0 - loop_prob) * pi[None, :])
        lpi = np.log(pi)
    lf = np.empty((t_rows, s))
    lb = np.zeros((t_rows, s))
    lf[0] = logp[0] + lpi
    for t in range(1, t_rows):
        lf[t] = logp[t] + _lse(lf[t - 1][:, None] + ltr, axis=0)
    for t in range(t_rows - 2, -1, -1):
        lb[t] = _lse(ltr + (logp[t + 1] + lb[t + 1])[None, :], axis=1)
    tll = float(_lse(lf[-1], axis=0))
    new_gamma = np.exp(lf + lb - tll)
    new_pi = new_gamma[0].copy()
    if t_rows > 1:
        prev = _lse(lf[:-1], axis=1)      # ln sum_i alpha_{t-1, i}
        new_pi += (1.0 - loop_prob) * pi * np.exp(prev[:, None] + logp[1:] + lb[1:] - tll).sum(axis=0)
    new_pi /= new_pi.sum()
    return new_gamma, new_pi, tll + second, tll, second


def iteration_scaled(x, phi, gamma, pi, loop_prob, fa, fb, dtype=np.float32):
    """One iteration in the per-frame scaled form, every array in `dtype`; tll and the ELBO's second term are accumulated in double from
    the dtype values.  A dead speaker (pi = 0) takes no part in the frame maximum and has b = 0.  -> as iteration_log."""
    dt = np.dtype(dtype)
    x, phi, gamma, pi = (np.asarray(a, dt) for a in (x, phi, gamma, pi))
    t_rows = x.shape[0]
    lp = dt.type(loop_prob)
    om = dt.type(1) - lp
    rho = x * np.sqrt(phi)[None, :]
    scores, second = speaker_models(rho, phi, gamma, fa, fb)
    live = pi > 0
    mx = np.where(live[None, :], scores, -np.inf).max(axis=1).astype(dt)
    b = np.where(live[None, :], np.exp(scores - mx[:, None]), dt.type(0)).astype(dt)
    ahat = np.empty_like(b)
    n = np.empty(t_rows, dt)
    a = b[0] * pi
    for t in range(t_rows):
        if t:
            a = b[t] * (lp * ahat[t - 1] + om * pi)
        n[t] = a.sum()
        ahat[t] = a / n[t]
    new_gamma = np.empty_like(b)
    beta = np.ones_like(pi)
    new_gamma[-1] = ahat[-1]
    acc = np.zeros_like(pi)
    for t in range(t_rows - 2, -1, -1):
        w = b[t + 1] * beta
        acc += w / n[t + 1]
        beta = (lp * w + om * (pi * w).sum()) / n[t + 1]
        new_gamma[t] = ahat[t] * beta
    new_pi = new_gamma[0] + om * pi * acc
    new_pi = (new_pi / new_pi.sum()).astype(dt)
    tll = float(np.sum(np.log(n.astype(np.float64)) + mx.astype(np.float64))) + frame_terms(x, fa)
    return new_gamma, new_pi, tll + second, tll, second


def vbx(x, phi, gamma, pi, loop_prob=0.99, fa=0.3, fb=17.0, max_iters=20, epsilon=1e-4, form="scaled", dtype=np.float64):
    """The whole operation for one recording.  -> (gamma, pi, ELBO list of the iterations run, labels)."""
    elbos = []
    for it in range(max_iters):
        if form == "log":
            gamma, pi, elbo = iteration_log(x, phi, gamma, pi, loop_prob, fa, fb)[:3]
        else:
            gamma, pi, elbo = iteration_scaled(x, phi, gamma, pi, loop_prob, fa, fb, dtype)[:3]
        elbos.append(elbo)
        if it > 0 and elbos[-1] - elbos[-2] < epsilon:
            break
    return gamma, pi, elbos, np.argmax(gamma, axis=1).astype(np.int32)


def first_appearance(labels):
    """Labels renumbered 0, 1, ... in order of first appearance: the clusterer's convention."""
    seen = {}
    return np.asarray([seen.setdefault(int(l), len(seen)) for l in labels], np.int32)


def make_case(t_rows, d, s, seed):
    """The inputs the GPU tests share: Phi = linspace(8, 0.1, D); k = max(1, S // 2) true speakers with means ~ N(0, diag Phi); rows =
    mean + N(0, I) in turns of 6 to 23 windows (the first k turns name every speaker once, where the recording is long enough); the start
    splits every true speaker in two by a coin (speaker i -> labels 2 i, 2 i + 1; S = 1: all 0), gives 10 % of the rows a random label
    among S, and applies smoothing 5.  -> dict(x float32 [T, D], phi float32 [D], gamma float32 [T, S], pi float32 [S], who int [T])."""
    from tf_kaldi_speaker_amd.misc.diarization import vbx_init
    rs = np.random.RandomState(1000 * seed + t_rows + 7 * d + 13 * s)
    phi = np.linspace(8.0, 0.1, d)
    k = max(1, s // 2)
    means = rs.randn(k, d) * np.sqrt(phi)[None, :]
    who = np.empty(t_rows, np.int64)
    at, turn = 0, 0
    while at < t_rows:
        length = int(rs.randint(6, 24))
        spk = turn if turn < k else int(rs.randint(0, k))
        who[at:at + length] = spk
        at, turn = at + length, turn + 1
    x = (means[who] + rs.randn(t_rows, d)).astype(np.float32)
    labels = (2 * who + rs.randint(0, 2, t_rows)) if s > 1 else np.zeros(t_rows, np.int64)
    noisy = rs.rand(t_rows) < 0.1
    labels = np.where(noisy, rs.randint(0, s, t_rows), labels)
    gamma = vbx_init(labels, s, 5.0)
    return dict(x=x, phi=phi.astype(np.float32), gamma=gamma, pi=np.full(s, 1.0 / s, np.float32), who=who)


def row_gap(gamma):
    """The smallest gap, over the rows, between the largest and the second largest responsibility (1 where S = 1)."""
    if gamma.shape[1] == 1:
        return 1.0
    top = np.sort(gamma, axis=1)
    return float((top[:, -1] - top[:, -2]).min())


# what the CPU and the GPU tests share: the shapes (T, D, S), the two parameter sets (fa, fb, loop_prob), and references computed once
SHAPES = ((1, 4, 1), (2, 4, 2), (65, 8, 4), (130, 16, 6), (257, 36, 7), (600, 128, 10), (2048, 256, 32))
PARAMS = ((0.3, 17.0, 0.99), (1.0, 1.0, 0.9))
_CACHE = {}


def case(shape, seed=0):
    key = ("case", shape, seed)
    if key not in _CACHE:
        c = make_case(*shape, seed=seed)
        for a in c.values():
            a.setflags(write=False)
        _CACHE[key] = c
    return _CACHE[key]


def one_iteration(shape, params, dtype, seed=0):
    """(gamma, pi, ELBO, tll, second term) of one scaled iteration on case(shape, seed) in `dtype`; computed once."""
    key = ("one", shape, params, np.dtype(dtype).name, seed)
    if key not in _CACHE:
        c, (fa, fb, lp) = case(shape, seed), params
        _CACHE[key] = iteration_scaled(c["x"], c["phi"], c["gamma"], c["pi"], lp, fa, fb, dtype)
    return _CACHE[key]


def converged(shape, seed, iters=20):
    """(gamma, labels, ELBO list) of `iters` float64 scaled iterations under PARAMS[0] on case(shape, seed), never stopped; computed once."""
    key = ("run", shape, seed, iters)
    if key not in _CACHE:
        c, (fa, fb, lp) = case(shape, seed), PARAMS[0]
        g, _, elbos, labels = vbx(c["x"], c["phi"], c["gamma"], c["pi"], lp, fa, fb, iters, -np.inf, "scaled", np.float64)
        _CACHE[key] = (g, labels, elbos)
    return _CACHE[key]


def gap_checked_seed(shape, iters=20):
    """The first seed whose float64 run ends with a gap of at least 0.5 between the two largest responsibilities of every row: a
    condition on the inputs (rounding cannot flip such a row), not a tolerance."""
    for seed in range(8):
        if row_gap(converged(shape, seed, iters)[0]) >= 0.5:
            return seed
    raise AssertionError("no seed of 0 .. 7 gives a gap of 0.5 at %r" % (shape,))
