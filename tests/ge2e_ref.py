"""NumPy restatement of the GE2E training loss (reference model/loss.py:903-982, its NumPy statement model/test_utils.py:21-86; kernels in
csrc/xv_triplet.hip; the arithmetic as include/xvector_hip.h states it), forward and backward, on the helpers of tests/triplet_ref.py - what
tests/test_ge2e_ref.py holds against the reference's oracle and tests/test_gpu_ge2e*.py compare the kernels with.

X is [B, D], B = N speakers x M segments, speaker-major; labels are not read.  l2(v) = v rsqrt(max(|v|^2, 1e-12)).

    x^_i = l2(x_i)      c^_k = l2(sum of speaker k's x^)      e^_i = l2(sum of the OTHER rows of i's speaker)
    c_ik = x^_i . c^_k (k != spk(i)),  c_i,own = x^_i . e^_i          S_ik = |w| c_ik + b
    softmax      mean_i [ logsumexp_k S_ik - S_i,own ]
    contrastive  mean_i [ 1 - sigmoid(S_i,own) + max(0, max_{k != own} sigmoid(S_ik)) ]      (N = 1: the 0 alone remains, without gradient)

`direct` states this as the TensorFlow body does, on the rows.  `ge2e` takes the kernels' route through u = X^ X^T (triplet_ref.cosine):
t_ik = sum_{m in k} u_im, n_k = sum_{m, m' in k} u_mm', and for the own speaker the same sums over the pairs that do not touch row i; every
formula takes a dtype: float64 is the reference, float32 the plain NumPy evaluation.  1 - sigmoid(S) is evaluated as sigmoid(-S), and the
contrastive maximum is taken where S is largest (the sigmoid is monotone); a tie goes to the lowest index.

Backward, P = d loss / d S: d w = sign(w) sum P c, d b = sum P (as that sum in both types), d X = A X with A from Q = d loss / d u as
triplet_ref.pair_loss forms it from its Q.  maximum(., 1e-12) passes no gradient to a clamped norm (passes at equality, as the pairwise
heads have it) and the numerator keeps its factor rsqrt(1e-12).

Bounds are those of DESIGN.md section 6h: u = 2^-24, a sum of terms with a longest addition chain L and c roundings per term is within
(L + c) u sum|terms| of the exact sum; an entry's bound is propagated through what is computed from it.  Decisions (`gap`, in bounds; a case
needs gap >= STABLE = 64): the runner-up of the contrastive maximum, and every clamp against 1e-12 - G_ii, n_k, the exclusive norm.  A norm
that is exactly 0 in any arithmetic is no decision: a zero row (its products are 0), and a speaker - or a speaker without one of its rows -
whose rows cancel in bit-negated pairs (G_ij and G_i'j then hold the same bits with opposite signs, r is equal, and the sums add them to 0 exactly)."""
import numpy as np

import triplet_ref as R

U, EPS, STABLE = R.U, R.EPS, R.STABLE
U64 = 2.0 ** -53
SOFTMAX, CONTRASTIVE = "softmax", "contrastive"
TYPES = (SOFTMAX, CONTRASTIVE)


def sigmoid(s, dt=np.float64):
    """1 / (1 + exp(-s)) without a difference of nearly equal numbers on either side (the kernel's sigmoid_f)"""
    s = np.asarray(s, dtype=dt)
    e = np.exp(-np.abs(s))
    hi = 1 / (1 + e)
    return np.where(s >= 0, hi, e * hi).astype(dt)


# ------------------------------------------------------------------ the TensorFlow body, on the rows (loss.py:921-982)
def direct(x, n, m, w, b, loss_type, dt=np.float64):
    x = np.asarray(x, dtype=dt)
    assert m != 1 and x.shape[0] == n * m
    rows = n * m
    xn = R.l2_scaling(x, dt)
    xr = xn.reshape(n, m, -1)
    center = R.l2_scaling(xr.sum(axis=1, dtype=dt), dt)
    center_ex = R.l2_scaling((xr.sum(axis=1, keepdims=True, dtype=dt) - xr).reshape(rows, -1), dt)
    sim = xn @ center.T
    own = np.repeat(np.arange(n), m)
    sim[np.arange(rows), own] = (xn * center_ex).sum(axis=1, dtype=dt)
    sim = dt(abs(w)) * sim + dt(b)
    if loss_type == SOFTMAX:
        top = sim.max(axis=1, keepdims=True)
        lse = np.log(np.exp(sim - top).sum(axis=1, dtype=dt)) + top[:, 0]
        return float((lse - sim[np.arange(rows), own]).mean(dtype=dt))
    if loss_type != CONTRASTIVE:
        raise ValueError("The GE2E only support softmax and contrastive loss")
    mask = own[:, None] == np.arange(n)[None, :]
    neg = ((1 - mask) * sigmoid(sim, dt)).max(axis=1)
    return float((sigmoid(-sim[np.arange(rows), own], dt) + neg).mean(dtype=dt))


# ------------------------------------------------------------------ the kernels' route
def cancels(block):
    """the rows of a speaker pair up as bit-negations of each other: their sum, and every sum over them of products with one row, is exactly 0"""
    block = np.asarray(block, np.float64)
    if block.shape[0] == 0 or block.shape[0] % 2 or np.abs(block.sum(axis=0)).max() != 0 or np.abs(block).sum() == 0:
        return False
    order = lambda a: a[np.lexsort(a.T[::-1])]
    return np.array_equal(order(block), order(-block))


def _ratio(dist, bound):
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(bound > 0, dist / np.where(bound > 0, bound, 1), np.where(dist > 0, np.inf, 0))
    return float(np.min(q)) if np.size(q) else np.inf


def ge2e(x, n, m, w, b, loss_type, backward=True, dt=np.float64):
    """-> Result(loss, dw, db, dx, rows_mag; bound, bound_dw, bound_db of the values; gap; the entries u, nk, ex, c, S, P and their bounds
    bu, bnk, bex, bc, bS, bP)"""
    assert loss_type in TYPES and m != 1
    x = np.asarray(x, dtype=dt)
    x64 = R.f64(x)
    rows, dim = x.shape
    assert rows == n * m
    own = np.repeat(np.arange(n), m)
    idx = np.arange(rows)
    g, r, u, _, _ = R.cosine(x, dt)
    bu = R.cosine_bound(x64)
    ur, bur = u.reshape(rows, n, m), bu.reshape(rows, n, m)
    t = ur.sum(axis=2, dtype=dt)
    bt = bur.sum(axis=2) + (m + 1) * U * np.abs(R.f64(ur)).sum(axis=2)
    blk = np.stack([u[k * m:(k + 1) * m, k * m:(k + 1) * m] for k in range(n)])
    bblk = np.stack([bu[k * m:(k + 1) * m, k * m:(k + 1) * m] for k in range(n)])
    exact0 = np.array([cancels(x64[k * m:(k + 1) * m]) for k in range(n)])
    nk = np.where(exact0, 0, blk.sum(axis=(1, 2), dtype=dt)).astype(dt)
    bnk = np.where(exact0, 0, bblk.sum(axis=(1, 2)) + (m * m // 64 + 9) * U * np.abs(R.f64(blk)).sum(axis=(1, 2)))
    other0 = exact0[None, :] & (own[:, None] != np.arange(n)[None, :])
    t, bt = np.where(other0, 0, t).astype(dt), np.where(other0, 0, bt)
    # the own speaker without row i: the pairs that do not touch i
    keep = np.arange(m)[None, :] != (idx % m)[:, None]                      # [rows, m]
    pair_keep = keep[:, :, None] & keep[:, None, :]                         # [rows, m, m]
    ex = (blk[own] * pair_keep).sum(axis=(1, 2), dtype=dt)
    bex = (bblk[own] * pair_keep).sum(axis=(1, 2)) + (m * m // 256 + 11) * U * (np.abs(R.f64(blk[own])) * pair_keep).sum(axis=(1, 2))
    te = (ur[idx, own] * keep).sum(axis=1, dtype=dt)
    bte = (bur[idx, own] * keep).sum(axis=1) + (m + 1) * U * (np.abs(R.f64(ur[idx, own])) * keep).sum(axis=1)
    ex0 = np.array([cancels(x64[own[i] * m:(own[i] + 1) * m][keep[i]]) for i in range(rows)])      # the other rows cancel: exactly 0, as above
    ex, bex, te, bte = np.where(ex0, 0, ex).astype(dt), np.where(ex0, 0, bex), np.where(ex0, 0, te).astype(dt), np.where(ex0, 0, bte)
    eps = dt(EPS)
    rc = (1 / np.sqrt(np.maximum(nk, eps))).astype(dt)
    re = (1 / np.sqrt(np.maximum(ex, eps))).astype(dt)
    c = (t * rc[None, :]).astype(dt)
    c[idx, own] = te * re
    nk64, ex64 = R.f64(nk), R.f64(ex)
    rel_k = np.where(nk64 >= EPS, 0.5 * bnk / np.maximum(nk64, EPS), 0) + 6 * U
    rel_e = np.where(ex64 >= EPS, 0.5 * bex / np.maximum(ex64, EPS), 0) + 6 * U
    bc = bt * R.f64(rc)[None, :] + np.abs(R.f64(c)) * rel_k[None, :]
    bc[idx, own] = bte * R.f64(re) + np.abs(R.f64(c[idx, own])) * rel_e
    # c_ik that is 0 in any arithmetic: a zero row's, and a row's against a speaker that cancels.  Such entries of a row (with w = 0: all) give
    # S_ik = b to the bit and tie everywhere alike: no decision between them, the lowest index takes the maximum
    zero_c = (R.f64(np.diag(g)) == 0)[:, None] | other0
    bc = np.where(zero_c, 0, bc)
    tied = zero_c | (float(w) == 0)
    aw = dt(abs(w))
    S = (aw * c + dt(b)).astype(dt)
    S64 = R.f64(S)
    bS = abs(w) * bc + 2 * U * (np.abs(abs(w) * R.f64(c)) + abs(b))
    # decisions: every clamp against 1e-12
    gii = R.f64(np.diag(g))
    gap = min(_ratio(np.abs(gii - EPS), np.diag(R.gram_bound(x64))), _ratio(np.abs(nk64 - EPS)[~exact0], bnk[~exact0]), _ratio(np.abs(ex64 - EPS), bex))
    onehot = own[:, None] == np.arange(n)[None, :]
    if loss_type == SOFTMAX:
        top = S.max(axis=1, keepdims=True)
        z = np.exp(S - top).sum(axis=1, dtype=dt)
        lse = np.log(z) + top[:, 0]
        row = lse - S[idx, own]
        soft = (np.exp(S - top) / z[:, None]).astype(dt)
        P = (soft - onehot).astype(dt)
        brow = (bS.max(axis=1) + bS[idx, own]) + 16 * U * (np.abs(R.f64(lse)) + np.abs(S64[idx, own]) + 1) + (n // 256 + 10) * U
        bP = R.f64(soft) * (bS + bS.max(axis=1, keepdims=True) + (n // 256 + 16) * U) + U * onehot
    else:
        sp, sn = sigmoid(S, dt), sigmoid(-S, dt)
        d = (sp * sn).astype(dt)
        P = np.where(onehot, -d, 0).astype(dt)
        row = sn[idx, own].copy()
        brow = 0.25 * bS[idx, own] + 8 * U * R.f64(row)
        if n > 1:
            masked = np.where(onehot, -np.inf, S)
            kb = masked.argmax(axis=1)
            P[idx, kb] = d[idx, kb]
            row = row + sp[idx, kb]
            brow = brow + 0.25 * bS[idx, kb] + 8 * U * R.f64(sp[idx, kb])
            for i in range(rows):      # the runner-up of the maximum
                others = ~onehot[i].copy()
                others[kb[i]] = False
                if tied[i, kb[i]]:
                    others &= ~tied[i]
                if others.any():
                    gap = min(gap, _ratio((S64[i, kb[i]] - S64[i, others]), (bS[i, others] + bS[i, kb[i]])))
        bP = np.abs(R.f64(P)) * (bS + 12 * U)
    loss = row.mean(dtype=dt)
    row64 = R.f64(row)
    Pc = R.f64(P) * R.f64(c)
    dw = dt(np.sign(w)) * (P * c).sum(dtype=dt) / dt(rows)
    db = P.sum(dtype=dt) / dt(rows)
    res = R.Result(loss=float(loss), dw=float(dw), db=float(db), dx=None, rows_mag=None, gap=gap,
                   bound=float(brow.mean() + (rows // 256 + 10) * U * np.abs(row64).mean()),
                   bound_dw=float(((bP * np.abs(R.f64(c)) + np.abs(R.f64(P)) * bc).sum() + (n // 256 + 12) * U * np.abs(Pc).sum()) / rows + 2 * U * abs(float(dw))),
                   bound_db=float((bP.sum() + (n // 256 + 10) * U * np.abs(R.f64(P)).sum()) / rows + 2 * U * abs(float(db))),
                   u=u, bu=bu, nk=nk, bnk=bnk, ex=ex, bex=bex, c=c, bc=bc, S=S, bS=bS, P=P, bP=bP)
    if not backward:
        return res
    # Q = d (sum of the row losses) / d u, every entry of u a variable of its own
    pc = P * c
    colsum = np.where(onehot, 0, pc).sum(axis=0, dtype=dt)                  # sum over the rows of the other speakers
    dn = np.where(nk >= eps, dt(-0.5) * aw * colsum / np.maximum(nk, eps), 0).astype(dt)
    de = np.where(ex >= eps, dt(-0.5) * aw * pc[idx, own] / np.maximum(ex, eps), 0).astype(dt)
    Q = (aw * P * rc[None, :])[:, own].astype(dt)                           # j in another speaker k: through t_ak
    loc = np.arange(m)
    not_a_j = (loc[None, None, :] != loc[:, None, None]) & (loc[None, None, :] != loc[None, :, None])      # [a, j, i]
    for k in range(n):
        sl = slice(k * m, (k + 1) * m)
        blockq = dn[k] + (not_a_j * de[sl][None, None, :]).sum(axis=2, dtype=dt)
        blockq = blockq + np.where(loc[:, None] != loc[None, :], (aw * P[sl, k] * re[sl])[:, None], 0)
        Q[sl, sl] = blockq
    a = (dt(1.0) / dt(rows)) * (Q + Q.T) * (r[:, None] * r[None, :])
    chain = np.where(np.diag(g) >= eps, -(r * r) * (a * g).sum(axis=1, dtype=dt), 0)
    res.dx = a @ x + chain[:, None] * x
    res.rows_mag = np.abs(R.f64(a + np.diag(chain))) @ np.abs(x64)
    return res


# ------------------------------------------------------------------ restatement against the reference's NumPy oracle
def oracle_eps_bound(x, n, m, w, b, loss_type):
    """What compute_ge2e_loss (model/test_utils.py:21-86) may differ by from `ge2e` in float64 on rows whose norms are not clamped: its
    epsilons are sqrt(. + 1e-16), / (... + 1e-16) and log(. + 1e-16) against max(., 1e-12), and it uses w where the loss has |w| (so w > 0).
      rows     x / sqrt(|x|^2 + 1e-16): a factor within rho_i = 0.5e-16 / |x_i|^2 of 1 / |x_i|; compute_cos divides by the norms again, so only
               the direction of a sum of such rows moves: by at most sum rho / |sum| (twice: numerator and the norm)
      centres  every pass of its loop over the speakers divides ALL centres by sqrt(|.|^2 + 1e-16) again; compute_cos normalises again: no effect
      cosine   / (|a| |b| + 1e-16) with |a|, |b| the norms after those scalings: c (1 - 1e-16 / (|a| |b|)), and |a| |b| >= (1 - 1e-15)
      log      log(p + 1e-16) against log p at the target's probability p: 1e-16 / p
    plus the float64 roundings of both evaluations: a cosine is a sum of D products over two sums of M rows, (D + 2 M + 16) 2^-53 of its terms.
    -> the bound of the loss value"""
    assert w > 0
    x = R.f64(x)
    rows, dim = x.shape
    res = ge2e(x, n, m, w, b, loss_type, backward=False)
    own = np.repeat(np.arange(n), m)
    idx = np.arange(rows)
    sq = (x * x).sum(axis=1)
    rho = 0.5e-16 / sq
    rho_k = rho.reshape(n, m).sum(axis=1)
    nk, ex = R.f64(res.nk), R.f64(res.ex)
    safe = lambda v: np.where(v > 0, 1 / np.sqrt(np.where(v > 0, v, 1)), 0)      # a sum that is exactly 0 gives c = 0 in both (0 / 1e-16)
    dc = np.abs(res.c) * (1e-16 * (1 + 1e-15) + rho[:, None]) + 2 * rho_k[None, :] * safe(nk)[None, :]
    dc[idx, own] = np.abs(res.c[idx, own]) * (1e-16 * (1 + 1e-15) + rho) + 2 * (rho_k[own] - rho) * safe(ex)
    dc = dc + (dim + 2 * m + 16) * U64 * (1 + np.abs(res.c))
    dS = abs(w) * dc + 2 * U64 * (np.abs(res.S) + abs(b))
    if loss_type == SOFTMAX:
        top = res.S.max(axis=1, keepdims=True)
        p = np.exp(res.S - top)[idx, own] / np.exp(res.S - top).sum(axis=1)
        drow = dS.max(axis=1) + dS[idx, own] + 1e-16 / p + (n + 16) * U64 * (np.abs(np.log(p)) + 1)
    else:
        drow = 0.25 * (dS.max(axis=1) + dS[idx, own]) + 16 * U64
    return float(drow.mean() + (rows + 2) * U64 * abs(res.loss))


# ------------------------------------------------------------------ cases
WB = ((10.0, -5.0), (20.0, 0.0), (1.0, 0.5))      # the reference's defaults; the validation loss's scale; a flat softmax
# (N, M, D, pitch of x beyond D, types): tests/test_gpu_ge2e.py; the contrastive maximum is a decision, so its largest case is 13 x 10
SHAPES = ((2, 2, 4, 4, TYPES), (1, 2, 8, 4, TYPES), (3, 2, 8, 4, TYPES), (4, 3, 512, 4, TYPES), (13, 10, 512, 4, TYPES), (39, 10, 512, 4, (SOFTMAX,)),
          (64, 10, 512, 4, (SOFTMAX,)))
OP_W, OP_B = 10.0, -5.0


def sized_case(n, m, dim, loss_type, w=OP_W, b=OP_B, first_seed=0, factor=1.0):
    """(seed, x) of the first decision-stable draw (gap >= factor * STABLE) of triplet_ref.embeddings(n, m, dim, seed, "randn")"""
    seed, (x, _) = R.stable_case(lambda s: R.embeddings(n, m, dim, s, "randn"),
                                 lambda case: ge2e(case[0], n, m, w, b, loss_type, backward=False).gap >= factor * STABLE, first_seed)
    return seed, x


def hostile_cases():
    """name -> (x [8, 16] float32 of 4 speakers x 2 segments, w, b); embeddings drawn in 8 dimensions and spread over the columns"""
    base, _ = R.embeddings(4, 2, 16, 3, "randn")
    out = {}
    x = base.copy(); x[3] = x[2]
    out["equal rows in a speaker"] = (x, OP_W, OP_B)
    x = base.copy(); x[5] = 0
    out["zero row"] = (x, OP_W, OP_B)
    x = base.copy(); x[3] = -x[2]
    out["x and -x"] = (x, OP_W, OP_B)
    out["w = -3"] = (base.copy(), -3.0, 0.5)
    out["w = 0"] = (base.copy(), 0.0, 0.5)
    out["|w| = 40, b = -20"] = (base.copy(), -40.0, -20.0)
    return out
