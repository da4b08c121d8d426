"""NumPy restatement of the pairwise loss heads (reference model/loss.py:358-705, model/common.py:61-110; kernels in csrc/xv_triplet.hip):
the semi-hard triplet loss, the angular triplet loss and the end-to-end validation loss, forward and (triplet losses) backward, with the
rounding bounds of the pair-matrix entries and of the loss values, and the decision-gap function - what tests/test_gpu_triplet*.py compare
the kernels with.

As in tests/attention_ref.py and tests/vlad_ref.py: every formula takes a dtype, float64 is the reference and float32 the plain NumPy
evaluation; u = 2^-24; a sum of terms t_i with a longest addition chain of L and c roundings per term is within (L + c) u sum|t_i| of the
exact sum.  With G = X X^T (the kernel sums the products of 16 columns with fused multiply-adds and adds these sums in order:
L = 16 + ceil(D / 16), one to spare):

    cosine     u_ij = G_ij (r_i r_j), r_i = 1 / sqrt(max(G_ii, 1e-12)), S = clip(u, -1, 1)
    Euclidean  D2_ij = max((G_ii - 2 G_ij) + G_jj, 0); squared: d = D2, else d = sqrt(D2) and 0 where D2 == 0

These losses are discontinuous in their decisions.  `Result.gap` is the smallest distance of a decision from its threshold in units of the
derived bound of the compared quantities; a test case must have gap >= STABLE (64), so that float32 takes every decision as float64 does.
Decisions: a hinge argument against 0 (and against 1e-12 in "all" mining), d_xy > d_xi, the runner-up of every min / max, |S| against 1 off the
diagonal, the arc threshold cos(pi - m), the asoftmax sign thresholds.  A hinge whose two sides are the SAME entry under the same transform
(an anchor without negatives in "hard" mining: hn = hp = min f) is identically 0 in any arithmetic and is no decision.

Stated rules of the backward: maximum(x, 0) passes at x >= 0, the clip passes at its bounds, the masked sqrt entries
get 0; a tie in a min / max gives the whole gradient to the LOWEST index (TensorFlow splits it); the arc margin's 1 - S^2 is clamped at 1e-12
in the derivative, so the gradient is finite at |S| = 1 (TensorFlow's is not).

Where no bound is derived - the sqrt near 0, the arc transform near |S| = 1 (Result.bounded is False), and d X, whose terms cancel -
`close_to_f32_eval` applies: the kernel may be 8 times as far from float64 as the float32 NumPy evaluation of the same formulas, per row,
and never has to be closer than 8 roundings of the row's largest sum of |terms|."""
import numpy as np

U = 2.0 ** -24
STABLE = 64.0
EPS = 1e-12
SEMIHARD, ALL, HARD = "semihard", "all", "hard"
MARGIN_KINDS = {"asoftmax": 1, "additive_margin_softmax": 2, "additive_angular_margin_softmax": 3}


def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def f64(a):
    return np.asarray(a, dtype=np.float64)


class Result(object):
    """loss, stats [3], dx (None for forward-only), bound (of the loss value), bounded (False: no derived bound exists), gap (see the module text)"""

    def __init__(self, **kw):
        self.__dict__.update(kw)


# ------------------------------------------------------------------ pair matrices
def same_rows(x):
    """[B, B]: rows i and j hold the same bits.  What is computed from such rows is the same number in the kernel (G_ij sums the same
    products in the same order) and here (gram), in either precision: a comparison between two such numbers comes out the same everywhere and
    is no decision, and a min / max over them goes to the lowest index everywhere."""
    _, inv = np.unique(np.asarray(x), axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    return inv[:, None] == inv[None, :]


def gram(x, dt):
    """X X^T on the distinct rows, symmetrised and spread out again: equal rows give equal entries, G_ij == G_ji (as the kernel's)."""
    x = np.asarray(x, dtype=dt)
    xu, inv = np.unique(x, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    gu = xu @ xu.T
    gu = np.triu(gu) + np.triu(gu, 1).T
    return gu[inv][:, inv]


GEMM_STEP = 16      # pair_gemm_kernel sums the products of 16 k on their own (fused multiply-adds) and adds each such sum once


def gemm_chain(k):
    return GEMM_STEP + -(-k // GEMM_STEP)


def gram_bound(x):
    """(16 + ceil(D / 16) + 1) u sum_c |x_ic x_jc|"""
    a = np.abs(f64(x))
    return (gemm_chain(x.shape[1]) + 1) * U * (a @ a.T)


def cosine(x, dt=np.float64):
    """-> (G, r, u, S, passes)"""
    g = gram(x, dt)
    r = (1.0 / np.sqrt(np.maximum(np.diag(g), dt(EPS)))).astype(dt)
    u = g * (r[:, None] * r[None, :])
    return g, r, u, np.clip(u, -1, 1), (u >= -1) & (u <= 1)


def cosine_bound(x):
    """|u - u64|: the entry of G scaled, plus u's own size times the relative error of r_i r_j (sqrt, division, one to spare each; the
    product and the scaling round once each)."""
    g, r, u, _, _ = cosine(x)
    bg = gram_bound(x)
    rho = 0.5 * np.diag(bg) / np.maximum(np.diag(g), EPS) + 3 * U
    return bg * (r[:, None] * r[None, :]) + np.abs(u) * (rho[:, None] + rho[None, :] + 2 * U)


def euclid(x, squared, dt=np.float64):
    """-> (G, d, chain = d d / d raw)"""
    g = gram(x, dt)
    sq = np.diag(g)
    raw = (sq[:, None] - 2 * g) + sq[None, :]
    d2 = np.maximum(raw, 0)
    ps = (raw >= 0).astype(dt)
    if squared:
        return g, d2, ps
    zero = d2 == 0
    d = np.where(zero, 0, np.sqrt(np.where(zero, 1, d2)))
    return g, d, np.where(zero, 0, ps * 0.5 / np.where(zero, 1, d))


def euclid_bound(x, squared):
    """-> (bound [B, B], bounded).  D2: the three entries of G and two roundings; sqrt: the bound of D2 over 2 d and two roundings of d, where
    D2 is at least STABLE bounds away from 0; an exact 0 between bit-identical rows (and the diagonal) is exact in any arithmetic."""
    x = f64(x)
    g, d, _ = euclid(x, squared)
    bg, sq = gram_bound(x), np.abs(np.diag(g))
    b2 = np.diag(bg)[:, None] + 2 * bg + np.diag(bg)[None, :] + 2 * U * (sq[:, None] + 2 * np.abs(g) + sq[None, :])
    same = same_rows(x)
    if squared:
        return np.where(same, 0, b2), True
    d2 = d * d
    ok = same | (d2 > STABLE * b2)
    return np.where(same, 0, b2 / (2 * np.maximum(d, 1e-300)) + 2 * U * d), bool(ok.all())


# ------------------------------------------------------------------ the positive side of the angular loss
def positive(s, margin_kind, m, dt=np.float64):
    """-> (f(S), f'(S)) of loss.py:537-560; tf.sign and the branch choices carry no gradient"""
    s = np.asarray(s, dtype=dt)
    if margin_kind == 1:
        if int(m) == 1:
            return s, np.ones_like(s)
        if int(m) == 2:
            return 2 * (np.sign(s) * (s * s)) - 1, 4 * np.sign(s) * s
        assert int(m) == 4, "[ERROR] m=%d is not unsupported if asoftmax is selected." % m
        c2 = s * s
        c4 = c2 * c2
        s0 = np.sign(s)
        s3 = np.sign(2 * c2 - 1) * s0
        return s3 * (8 * c4 - 8 * c2 + 1) + (2 * s0 + s3 - 3), s3 * (32 * c2 * s - 16 * s)
    if margin_kind == 2:
        return s - dt(m), np.ones_like(s)
    cm, sm, th = dt(np.cos(m)), dt(np.sin(m)), dt(np.cos(np.pi - m))
    q = 1 - s * s
    nf = s * cm - np.sqrt(np.maximum(q, 0)) * sm
    nd = cm + s / np.sqrt(np.maximum(q, dt(EPS))) * sm
    easy = s <= th
    return np.where(easy, -nf - 2, nf), np.where(easy, -nd, nd)


def positive_bound(s, bs, margin_kind, m):
    """-> (|f - f64| [B, B], bounded [B, B]): |f'| bs plus the roundings of the transform itself"""
    s = f64(s)
    f, df = positive(s, margin_kind, m)
    ok = np.ones(s.shape, bool)
    if margin_kind == 1 and int(m) == 1:
        return bs, ok
    if margin_kind == 1 and int(m) == 2:
        own = 3 * U * (2 * s * s + 1)
    elif margin_kind == 1:
        own = 8 * U * (8 * s ** 4 + 8 * s * s + 4)
    elif margin_kind == 2:
        own = U * (np.abs(s) + abs(m))
    else:
        # sqrt(1 - S^2): with the slope where it is moderate; near |S| = 1 (the diagonal, equal rows) |sqrt(q') - sqrt(q)| <= sqrt(|q' - q|)
        q = np.maximum(1 - s * s, 0)
        rq = np.sqrt(np.maximum(q, 1e-30))
        dq = 2 * np.abs(s) * bs + 3 * U
        broot = np.minimum(dq / (2 * rq) + U * rq, np.sqrt(dq) + U * rq)
        return abs(np.cos(m)) * bs + abs(np.sin(m)) * broot + U * (2 * np.abs(s * np.cos(m)) + 2 * abs(np.sin(m)) * rq + 2 * np.abs(f) + 2), ok
    return np.abs(df) * bs + own, ok


def thresholds_gap(s, bs, margin_kind, m, same):
    """distance of every S between two different rows from the values at which f branches (and from the clip's bounds), in bounds"""
    s = f64(s)
    off = ~same
    if not off.any():
        return np.inf
    marks = [1.0, -1.0]
    if margin_kind == 1 and int(m) >= 2:
        marks.append(0.0)
    if margin_kind == 1 and int(m) == 4:
        marks += [np.sqrt(0.5), -np.sqrt(0.5)]
    if margin_kind == 3:
        marks.append(np.cos(np.pi - m))
    return min((np.abs(s - t)[off] / bs[off]).min() for t in marks)


# ------------------------------------------------------------------ mining
def _runner_up(values, best, bound, best_bound, smallest, dup):
    """gap, in bounds, between the chosen value of a min (smallest) / max and the next candidate that is not the same row (dup) as the chosen one"""
    keep = ~dup
    keep[best] = False
    others = values[keep]
    if others.size == 0:
        return np.inf
    diff = (others - values[best]) if smallest else (values[best] - others)
    return (diff / (bound[keep] + best_bound)).min()


def semihard_mine(d, bd, labels, margin, same, dt=np.float64):
    """-> (sum, pairs, Q = d sum / d d [B, B], sum of the terms' bounds, sum |terms|, gap)"""
    b = d.shape[0]
    q = np.zeros((b, b), dt)
    total, pairs, bsum, asum, gap = dt(0), 0, 0.0, 0.0, np.inf
    for x in range(b):
        row, rb = d[x], bd[x]
        neg = labels != labels[x]
        for i in np.nonzero((labels == labels[x]) & (np.arange(b) != x))[0]:
            out = np.nonzero(neg & (row > row[i]))[0]
            cmpd = neg & ~same[i]
            if cmpd.any():
                gap = min(gap, (np.abs(row[cmpd] - row[i]) / (rb[cmpd] + rb[i])).min())
            if out.size:
                k = np.argmin(row[out]); y = out[k]
                gap = min(gap, _runner_up(row[out], k, rb[out], rb[y], True, same[y][out]))
            elif neg.any():
                cand = np.nonzero(neg)[0]
                k = np.argmax(row[cand]); y = cand[k]
                gap = min(gap, _runner_up(row[cand], k, rb[cand], rb[y], False, same[y][cand]))
            else:
                y = int(np.argmin(row))
                gap = min(gap, _runner_up(row, y, rb, rb[y], True, same[y]))
            t = dt(margin) + (row[i] - row[y])
            tb = rb[i] + rb[y] + 2 * U * (abs(margin) + abs(row[i]) + abs(row[y]))
            gap = min(gap, abs(t) / tb)
            pairs += 1
            if t >= 0:
                total += t
                q[x, i] += 1
                q[x, y] -= 1
                bsum += tb
                asum += abs(t)
    return total, pairs, q, bsum, asum, gap


def angular_mine(s, f, df, bs, bf, labels, triplet_type, dup, identity, dt=np.float64):
    """-> (sum, valid, positive, Q = d sum / d S [B, B], sum of the terms' bounds, sum |terms|, gap)"""
    b = s.shape[0]
    q = np.zeros((b, b), dt)
    total, valid, npos, bsum, asum, gap = dt(0), 0, 0, 0.0, 0.0, np.inf
    idx = np.arange(b)
    for a in range(b):
        same = labels == labels[a]
        pos, neg = np.nonzero(same & (idx != a))[0], np.nonzero(~same)[0]
        if triplet_type == ALL:
            if pos.size == 0 or neg.size == 0:
                continue
            t = s[a, neg][None, :] - f[a, pos][:, None]
            tb = bs[a, neg][None, :] + bf[a, pos][:, None] + U * (np.abs(s[a, neg])[None, :] + np.abs(f[a, pos])[:, None])
            dec = ~dup[pos][:, neg] if identity else np.ones(t.shape, bool)      # f = identity on one number: S - S = 0 everywhere
            if dec.any():
                gap = min(gap, (np.abs(t) / tb)[dec].min(), (np.abs(t - EPS) / tb)[dec].min())
            act = t >= 0
            valid += t.size
            npos += int((t > EPS).sum())
            total += t[act].sum(dtype=dt)
            bsum += tb[act].sum()
            asum += np.abs(t[act]).sum()
            q[a, neg] += act.sum(axis=0)
            q[a, pos] -= act.sum(axis=1) * df[a, pos]
            continue
        fa, ba = f[a], bf[a]
        imax, imin = int(np.argmax(fa)), int(np.argmin(fa))
        if pos.size == 0:      # the fillers decide only where they are used
            gap = min(gap, _runner_up(fa, imax, ba, ba[imax], False, dup[imax]))
        if neg.size == 0:
            gap = min(gap, _runner_up(fa, imin, ba, ba[imin], True, dup[imin]))
        real_p = same & (idx != a)
        ap = np.where(real_p, fa, fa[imax])
        an = np.where(same, fa[imin], s[a])
        apb, anb = np.where(real_p, ba, ba[imax]), np.where(same, ba[imin], bs[a])
        ip, jn = int(np.argmin(ap)), int(np.argmax(an))
        if pos.size:      # among the real candidates only: the fillers repeat one value
            k = int(np.argmin(fa[pos]))
            gap = min(gap, _runner_up(fa[pos], k, ba[pos], apb[ip], True, dup[pos[k]][pos]))
        if neg.size:
            k = int(np.argmax(s[a, neg]))
            gap = min(gap, _runner_up(s[a, neg], k, bs[a, neg], anb[jn], False, dup[neg[k]][neg]))
        t = an[jn] - ap[ip]
        jp, jq = (ip if real_p[ip] else imax), (jn if not same[jn] else imin)
        identical = (jp == jq and same[jn]) or (identity and not same[jn] and real_p[ip] and dup[jn, ip])      # one number on both sides
        tb = apb[ip] + anb[jn] + U * (abs(an[jn]) + abs(ap[ip]))
        if not identical:
            gap = min(gap, abs(t) / tb)
        valid += 1
        npos += int(t > 0)
        if t >= 0:
            total += t
            bsum += 0 if identical else tb
            asum += abs(t)
            q[a, jp] -= df[a, jp]
            q[a, jq] += 1 if not same[jn] else df[a, jq]
    return total, valid, npos, q, bsum, asum, gap


# ------------------------------------------------------------------ the two triplet losses
def pair_loss(x, labels, kind, margin=0.0, squared=False, margin_kind=2, backward=True, dt=np.float64):
    """kind: SEMIHARD | ALL | HARD (the angular loss with that triplet_type) -> Result"""
    x = np.asarray(x, dtype=dt)
    labels = np.asarray(labels)
    b, dim = x.shape
    x64 = f64(x)
    dup = same_rows(x)
    if kind == SEMIHARD:
        g, d, chain = euclid(x, squared, dt)
        bd, bounded = euclid_bound(x64, squared)
        total, pairs, q, bsum, asum, gap = semihard_mine(d, bd, labels, margin, dup, dt)
        den = max(float(pairs), 1e-16)
        stats = [float(pairs), 0.0, 0.0]
        chain_len = 4 + 8 + 2
        qraw = q * chain
    else:
        g, r, u, s, passes = cosine(x, dt)
        bs = cosine_bound(x64)
        f, df = positive(s, margin_kind, margin, dt)
        bf, okf = positive_bound(f64(s), bs, margin_kind, margin)
        bounded = bool(okf[~dup].all()) if (~dup).any() else True
        if kind == HARD and margin_kind == 3 and (np.unique(labels, return_counts=True)[1] == 1).any():
            bounded = False      # an anchor without a positive takes f(S_aa): the arc transform at |S| = 1
        total, valid, npos, q, bsum, asum, gap = angular_mine(s, f, df, bs, bf, labels, kind, dup, margin_kind == 1 and int(margin) == 1, dt)
        gap = min(gap, thresholds_gap(s, bs, margin_kind, margin, dup))
        den = (npos + 1e-16) if kind == ALL else float(b)
        stats = [float(valid), float(npos), npos / (valid + 1e-16) if kind == ALL else npos / float(b)]
        chain_len = 4 * b + 8 + 2
        qraw = q * passes
    loss = dt(total) / dt(den)
    res = Result(loss=float(loss), stats=stats, bound=(bsum + chain_len * U * asum) / den + 2 * U * abs(float(loss)), bounded=bounded, gap=gap,
                 dx=None, rows_mag=None)
    if not backward:
        return res
    scale = dt(1.0) / dt(den)
    if kind == SEMIHARD:
        dg = -2 * scale * qraw
        both = qraw.sum(axis=1) + qraw.sum(axis=0)
        dg[np.arange(b), np.arange(b)] += scale * both
        a = dg + dg.T
        res.dx = a @ x
    else:
        a = scale * (qraw + qraw.T) * (r[:, None] * r[None, :])
        c = np.where(np.diag(g) >= dt(EPS), -(r * r) * (a * g).sum(axis=1), 0)
        res.dx = a @ x + c[:, None] * x
        a = a + np.diag(c)
    res.rows_mag = np.abs(f64(a)) @ np.abs(x64)      # sum_j |A_ij x_jc|: what d X's roundings scale with
    return res


def close_to_f32_eval(got, ref64, eval32, mag, chain):
    """The rule for d X (module text): per row, |got - ref64| <= max(8 max|eval32 - ref64|, 8 (chain + 2) u max_c sum_j |A_ij x_jc|).
    The floor is not vlad_ref's 8 u max|ref|: a row of d X is a sum of B terms A_ij x_j that cancel (the gradient of a cosine is projected off its own
    row), so its rounding scales with sum |terms| and the length of the addition chain, not with the result - (chain + 2) u sum |terms| is the
    product's own bound - and A carries the entry errors of S through f' on top.  (With 8 u max|ref| one of the 192 sized cases, asoftmax m = 4 at
    130 x 4, lies at 1.04 of the allowance on an MI355X.)  -> (ok, largest error / tolerance)"""
    err = np.abs(f64(got) - ref64).max(axis=1)
    tol = np.maximum(8 * np.abs(f64(eval32) - ref64).max(axis=1), 8 * (chain + 2) * U * mag.max(axis=1)) + 1e-37
    return bool((err <= tol).all()), float((err / tol).max())


# ------------------------------------------------------------------ e2e validation loss, as loss.py:666-702 states it (not through G)
def l2_scaling(x, dt):
    return x * (1.0 / np.sqrt(np.maximum((x * x).sum(axis=-1, keepdims=True, dtype=dt), dt(EPS)))).astype(dt)


def e2e_valid_loss(x, speakers, segments, dt=np.float64):
    x = np.asarray(x, dtype=dt)
    n, m = int(speakers), int(segments)
    assert x.shape[0] == n * m
    xn = l2_scaling(x, dt)
    xr = xn.reshape(n, m, -1)
    center = l2_scaling(xr.mean(axis=1, dtype=dt), dt)
    center_ex = l2_scaling((xr.sum(axis=1, keepdims=True, dtype=dt) - xr).reshape(n * m, -1), dt)
    sim = xn @ center.T
    own = np.repeat(np.arange(n), m)
    sim[np.arange(n * m), own] = (xn * center_ex).sum(axis=1, dtype=dt)
    sim = dt(20) * sim
    top = sim.max(axis=1, keepdims=True)
    lse = np.log(np.exp(sim - top).sum(axis=1, dtype=dt)) + top[:, 0]
    return float((lse - sim[np.arange(n * m), own]).mean(dtype=dt))


def e2e_valid_bound(x, speakers, segments):
    """The kernel's route: u_ij as in the cosine matrix; a_is = sum_{m in s} u_im (M terms in order); n_s = sum over the speaker's M^2 pairs (a
    lane's M^2 / 64 terms, six butterfly steps; the own speaker's sum without row i: M^2 / 256 and a tree of 8); sim = a / sqrt(n) with the
    bound of n over 2 n and 4 roundings; the row's cross-entropy is 1-Lipschitz in every logit (x 20), its exp / log / sum add 16 roundings of
    the values and the chain of the N terms; the mean adds the chain of the B rows."""
    x = f64(x)
    n, m = int(speakers), int(segments)
    b = n * m
    _, _, u, _, _ = cosine(x)
    bu = cosine_bound(x)
    own = np.repeat(np.arange(n), m)
    ur, br = u.reshape(b, n, m), bu.reshape(b, n, m)
    a = ur.sum(axis=2)
    ba = br.sum(axis=2) + (m + 1) * U * np.abs(ur).sum(axis=2)
    blk_u = np.stack([u[s * m:(s + 1) * m, s * m:(s + 1) * m] for s in range(n)])
    blk_b = np.stack([bu[s * m:(s + 1) * m, s * m:(s + 1) * m] for s in range(n)])
    ns = blk_u.sum(axis=(1, 2))
    bn = blk_b.sum(axis=(1, 2)) + (m * m // 64 + 9) * U * np.abs(blk_u).sum(axis=(1, 2))
    sim = a / np.sqrt(np.maximum(ns, EPS * m * m))[None, :]
    bsim = ba / np.sqrt(np.maximum(ns, EPS * m * m))[None, :] + np.abs(sim) * (0.5 * bn / np.maximum(ns, EPS * m * m) + 6 * U)[None, :]
    for i in range(b):
        s, k = own[i], i % m
        keep = np.arange(m) != k
        ex = blk_u[s][keep][:, keep].sum()
        bex = blk_b[s][keep][:, keep].sum() + (m * m // 256 + 11) * U * np.abs(blk_u[s][keep][:, keep]).sum()
        dot = ur[i, s][keep].sum()
        bdot = br[i, s][keep].sum() + (m + 1) * U * np.abs(ur[i, s][keep]).sum()
        den = max(ex, EPS)
        sim[i, s] = dot / np.sqrt(den)
        bsim[i, s] = bdot / np.sqrt(den) + abs(sim[i, s]) * (0.5 * bex / den + 6 * U)
    logit = 20 * sim
    top = logit.max(axis=1)
    lse = np.log(np.exp(logit - top[:, None]).sum(axis=1)) + top
    row = lse - logit[np.arange(b), own]
    brow = 20 * (bsim.max(axis=1) + bsim[np.arange(b), own]) + 16 * U * (np.abs(lse) + np.abs(logit[np.arange(b), own]) + 1) + (n // 256 + 10) * U
    return float(brow.mean() + (b // 256 + 10) * U * np.abs(row).mean())


# ------------------------------------------------------------------ case generation (tests and the golden's generator share it)
def embeddings(speakers, segments, dim, seed, sign="rand"):
    """[speakers * segments, dim] float32, speaker-major, and the labels in blocks: `rand` (no negative entry, as the reference's self-test draws
    them; the 8th power keeps the rows from being all alike) or `randn` (mixed signs: the asoftmax sign branches and the arc easy-margin
    branch are taken), plus a speaker offset.  Drawn in min(dim, 8) dimensions and spread over the dim columns in blocks with weights
    0.5 .. 1.5: similarities of rows drawn in 512 dimensions lie within 1 / sqrt(512) of each other, too close for any seed to keep some
    hundred decisions 64 bounds apart."""
    rs = np.random.RandomState(seed)
    n, lat = speakers * segments, min(dim, 8)
    draw = (lambda *s: rs.rand(*s) ** 8) if sign == "rand" else rs.randn
    z = draw(n, lat) + np.repeat(draw(speakers, lat), segments, axis=0)
    spread = (0.5 + rs.rand(lat, dim)) * (np.arange(dim)[None, :] * lat // dim == np.arange(lat)[:, None])
    return f32(z @ spread), np.repeat(np.arange(speakers), segments).astype(np.int32)


def stable_case(make, check, first_seed=0, tries=200):
    """The first seed >= first_seed whose case check(case) accepts (decision gap >= STABLE in every configuration the caller runs): an
    unstable draw is replaced at generation time, never skipped at run time."""
    for seed in range(first_seed, first_seed + tries):
        case = make(seed)
        if check(case):
            return seed, case
    raise AssertionError("no decision-stable case in %d seeds" % tries)


# ------------------------------------------------------------------ the cases of tests/test_gpu_triplet*.py
CONFIGS = ([("semihard/squared=%d" % sq, SEMIHARD, dict(margin=0.2, squared=bool(sq))) for sq in (1, 0)] +
           [("angular/%s/%s/%g" % (tt, lt, m), tt, dict(margin=m, margin_kind=MARGIN_KINDS[lt])) for tt in (ALL, HARD)
            for lt, m in (("asoftmax", 1.0), ("asoftmax", 2.0), ("asoftmax", 4.0), ("additive_margin_softmax", 0.1),
                          ("additive_angular_margin_softmax", 0.3))])
SIZES = (2, 4, 12, 15, 130)


def unit_rows(x):
    x = f64(x)
    return f32(x / np.sqrt((x * x).sum(axis=1, keepdims=True)))


def sized_case(b, dim, seed, kind):
    """(x float32 [b, dim], labels int32 [b]) of mixed sign; unit rows for the semi-hard loss (which expects them, loss.py:373).
        2    one speaker (no negatives)                    4    2 x 2                    12    4 x 3
        15   groups of 2, 3, 4 and 6 in a shuffled order (labels not speaker-major)
        130  13 rows (groups of 3, 4 and 6) ten times over, every copy under labels of its own: 30 speakers, more than one wave of anchors.
             130 rows drawn independently hold some 10^5 hinge arguments and cannot keep them all 64 bounds from 0; copies repeat the
             decisions of the 13 rows, and what is computed from equal rows is equal everywhere (same_rows).
        390  the same 13 rows thirty times over: columns 256 .. 389 are a thread's second column, and the ballot runs seven times"""
    if b == 15:
        x, lab = embeddings(4, 6, dim, seed, "randn")
        keep = np.concatenate([np.arange(6 * g, 6 * g + n) for g, n in enumerate((2, 3, 4, 6))])
        keep = keep[np.random.RandomState(seed + 1000).permutation(keep.size)]
        x, lab = x[keep], (7 * lab[keep] + 3).astype(np.int32)
    elif b % 13 == 0:
        x, _ = embeddings(1, 13, dim, seed, "randn")
        base = np.repeat([0, 1, 2], [3, 4, 6])
        x, lab = np.tile(x, (b // 13, 1)), np.concatenate([base + 3 * c for c in range(b // 13)]).astype(np.int32)
    else:
        x, lab = embeddings(*{2: (1, 2), 4: (2, 2), 12: (4, 3)}[b], dim, seed, "randn")
    return (unit_rows(x) if kind == SEMIHARD else f32(x)), lab
