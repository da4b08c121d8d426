"""Op-level wrappers of the pipeline stages around the network that take feature matrices or vectors (include/xvector_hip.h): the extraction
front end, the 'CM ' codec, cosine / AS-norm scoring and the LDA / PLDA back end with its cohort statistics; those that take PCM are in
wave_ops.py.  ops.py re-exports every public name here: callers write ops.score_trials.  Their kernels check none of the index arrays
they are handed, so much of this is validation (_host.host_ints) in front of one upload."""
import ctypes as C

import numpy as np
import torch

try:
    from ._host import _lib, _p, _s, exclusive_offsets, f32_values, host_ints, pitch4, pitched, spans_inside, upload
except ImportError:
    from _host import _lib, _p, _s, exclusive_offsets, f32_values, host_ints, pitch4, pitched, spans_inside, upload


def frontend(x, rows_in, cmn_window=0, masks=None, mask_offsets=None, first=None, count=None, t_out=None):
    """Sliding-window CMN (cmn_window frames, 0 = off), then voiced-frame selection, on a decoded batch x [b, t_in, d] with rows_in[i] raw
    frames per piece (xv_frontend).  masks: uint8 device tensor, the pieces' voicing masks back to back, piece i's at byte
    mask_offsets[i] (int64) - None keeps every frame; first / count (int32, None = 0 / t_out): the range of SELECTED rows a piece
    keeps.  -> (out [b, t_out, d], rows_out int32 [b])."""
    b, t_in, d = x.shape
    t_out = t_in if t_out is None else int(t_out)
    out = torch.empty((b, t_out, d), dtype=torch.float32, device=x.device)
    rows_out = torch.empty(b, dtype=torch.int32, device=x.device)
    ws = torch.empty((b, t_out), dtype=torch.int32, device=x.device) if masks is not None else None
    _lib.call("xv_frontend", _s(), _p(x), _p(rows_in), b, t_in, d, int(cmn_window), _p(masks), C.c_size_t(masks.numel() if masks is not None else 0),
              _p(mask_offsets), _p(first), _p(count), t_out, _p(out), _p(rows_out), _p(ws), C.c_size_t(ws.numel() * 4 if ws is not None else 0))
    return out, rows_out


CM_MAX_D = 128      # the columns the 'CM ' kernels take (CMD_MAX_D / CME_MAX_D)


def cm_decode_ragged(packed, offsets, rows, t, d):
    """'CM ' matrices as they sit in an archive behind the "CM " token, decoded on the device (xv_cm_decode_ragged; no Engine needed).
    packed: uint8 device tensor; offsets / rows: HOST integer arrays [b] - image i starts at byte offsets[i] and holds rows[i] <= t frames of d
    columns; they are checked here, before the upload.  -> float32 [b, t, d], the rows behind rows[i] zero."""
    if packed.dtype != torch.uint8 or packed.dim() != 1 or not packed.is_contiguous():
        raise ValueError("cm_decode_ragged: packed must be a contiguous 1-D uint8 tensor")
    t, d = int(t), int(d)
    if not 1 <= d <= CM_MAX_D:
        raise ValueError("cm_decode_ragged: d must lie in 1 .. %d (got %d)" % (CM_MAX_D, d))
    pair = "cm_decode_ragged: offsets and rows must be two non-empty 1-D integer arrays of one length"
    offsets = host_ints(offsets, min_size=1, msg=pair, dtype=np.int64)
    rows = host_ints(rows, "cm_decode_ragged: rows", n=offsets.size, lo=0, hi=t + 1, msg=pair, dtype=np.int64)
    spans_inside(offsets, cm_image_bytes(rows, d), packed.numel(), "cm_decode_ragged: an image lies outside the %d bytes of packed" % packed.numel())
    out = torch.empty((offsets.size, t, d), dtype=torch.float32, device=packed.device)
    off_d, rows_d = upload(offsets, np.int64, packed.device), upload(rows, np.int32, packed.device)
    _lib.call("xv_cm_decode_ragged", _s(), _p(packed), _p(off_d), _p(rows_d), offsets.size, t, d, _p(out))
    return out


def cm_image_bytes(rows, d):      # bytes of a 'CM ' matrix behind its token: global header, d column headers, d x rows codes
    return 16 + 8 * int(d) + int(d) * np.asarray(rows, np.int64)


def cm_encode_plan(shape, rows, header="quartiles"):
    """The checks and the offset arithmetic of cm_encode, on the host: shape = (b, t, d) of x -> (rows int32 [b], offsets int64 [b] of the
    images packed back to back, total bytes, the header's code).  Refuses by name: an unknown header, d > 128, rows[i] outside 1 .. t."""
    if header not in _lib.XV_CM_HEADERS:
        raise ValueError("cm_encode: header must be 'quartiles' or 'uniform' (got %r)" % (header,))
    b, t, d = (int(n) for n in shape)
    if not 1 <= d <= CM_MAX_D:
        raise ValueError("cm_encode: d must lie in 1 .. %d (got %d)" % (CM_MAX_D, d))
    rows = host_ints(rows, "cm_encode: rows", n=b, min_size=1, lo=1, hi=t + 1)
    sizes = cm_image_bytes(rows, d)
    return rows.astype(np.int32), exclusive_offsets(sizes), int(sizes.sum()), _lib.XV_CM_HEADERS[header]


def cm_encode(x, rows, header="quartiles"):
    """'CM ' compression of a padded batch on the device (xv_cm_encode: dataset.kaldi_io.write_compressed_mat byte for byte, in both header
    forms).  x: float32 [b, t, d] device tensor, piece i holding rows[i] frames; rows: a HOST integer array, checked here before the upload
    (1 <= rows[i] <= t; d <= 128; the header's name).  -> (uint8 device tensor: the images behind the "CM " token, packed back to back; their
    int64 host offsets [b]); image i has cm_image_bytes(rows[i], d) bytes."""
    if x.dim() != 3 or x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError("cm_encode: x must be a contiguous float32 [b, t, d] tensor")
    rows, offsets, total, code = cm_encode_plan(x.shape, rows, header)
    b, t, d = x.shape
    out = torch.empty(total, dtype=torch.uint8, device=x.device)
    rows_d, off_d = upload(rows, np.int32, x.device), upload(offsets, np.int64, x.device)
    _lib.call("xv_cm_encode", _s(), _p(x), _p(rows_d), b, t, d, code, _p(off_d), _p(out))
    return out, offsets


def _centered(name, entry, x, d, mean, out):      # score_prepare and backend_center: one row-wise kernel each, on the same arguments
    rows, ldx = pitched(x, "%s: x" % name)
    d = x.shape[1] if d is None else int(d)
    if out is None:
        out = torch.empty((rows, pitch4(d)), dtype=torch.float32, device=x.device)
    _, ldy = pitched(out, "%s: out" % name, whole=True)
    if mean is not None:
        f32_values(mean, d, "%s: mean" % name)
    _lib.call(entry, _s(), _p(x), rows, d, ldx, _p(mean), _p(out), ldy)
    return out


def score_prepare(x, d=None, mean=None, out=None):
    """Rows of x [rows, >= d] minus mean [d] (None: nothing subtracted), scaled to unit length (xv_score_prepare).  d: the columns that
    hold the vector (default: all of x).  out: the [rows, ldy] tensor to write (may be x itself, in place); default a new tensor whose
    pitch is d rounded up to 4 - columns d .. ldy come back zero, so the result is a GEMM operand for score_cohort_stats."""
    return _centered("score_prepare", "xv_score_prepare", x, d, mean, out)


def score_trials(e, t, d, ei, ti, e_stats=None, t_stats=None):
    """out[j] = e[ei[j]][:d] . t[ti[j]][:d], AS-normalised with the rows' cohort statistics when both are given (xv_score_trials).
    ei, ti: HOST integer arrays (NumPy / sequences): the kernel does not check indices, so they are checked here, before the upload."""
    ne, lde = pitched(e, "score_trials: e")
    nt, ldt = pitched(t, "score_trials: t")
    pair = "score_trials: ei and ti must be two non-empty 1-D integer arrays of one length"
    ei = host_ints(ei, min_size=1, msg=pair)
    ti = host_ints(ti, n=ei.size, msg=pair)
    if ei.min() < 0 or ei.max() >= ne:
        raise IndexError("score_trials: ei holds an index outside 0 .. %d" % (ne - 1))
    if ti.min() < 0 or ti.max() >= nt:
        raise IndexError("score_trials: ti holds an index outside 0 .. %d" % (nt - 1))
    for st, n, name in ((e_stats, ne, "e_stats"), (t_stats, nt, "t_stats")):
        if st is not None and (st.dtype != torch.float32 or tuple(st.shape) != (n, 2) or not st.is_contiguous()):
            raise ValueError("score_trials: %s must be a contiguous float32 [%d, 2] tensor" % (name, n))
    ei_d, ti_d = upload(ei, np.int32, e.device), upload(ti, np.int32, e.device)
    out = torch.empty(ei.size, dtype=torch.float32, device=e.device)
    _lib.call("xv_score_trials", _s(), _p(e), lde, ne, _p(t), ldt, nt, int(d), _p(ei_d), _p(ti_d), C.c_int64(ei.size), _p(e_stats), _p(t_stats),
              _p(out))
    return out


def score_cohort_workspace_bytes(rows, n_cohort, d):
    return int(_lib.load().xv_score_cohort_workspace_bytes(int(rows), int(n_cohort), int(d)))


def score_cohort_stats(x, cohort, d, top_k, ws_bytes=None):
    """[rows, 2] = (mean, biased deviation) of each row's min(top_k, n_cohort) largest scores against the cohort rows
    (xv_score_cohort_stats).  x, cohort: prepared matrices (score_prepare: zero padding up to a pitch that is a multiple of 4).
    ws_bytes: size of the score slab (default: the whole call in one GEMM launch); fewer bytes run the rows in tiles."""
    rows, ldx = pitched(x, "score_cohort_stats: x")
    n_cohort, ldc = pitched(cohort, "score_cohort_stats: cohort")
    if ws_bytes is None:
        ws_bytes = score_cohort_workspace_bytes(rows, n_cohort, d)
    ws = torch.empty(max(int(ws_bytes) // 4, 1), dtype=torch.float32, device=x.device)
    stats = torch.empty((rows, 2), dtype=torch.float32, device=x.device)
    _lib.call("xv_score_cohort_stats", _s(), _p(x), ldx, rows, _p(cohort), ldc, n_cohort, int(d), int(top_k), _p(stats), _p(ws),
              C.c_size_t(int(ws_bytes)))
    return stats


def backend_group_means(x, d, offsets, rows, want32=True):
    """Averages of groups of rows of x [n, >= d] (xv_backend_group_means): group g = rows[offsets[g]:offsets[g + 1]], added in list order in
    double.  offsets, rows: HOST integer arrays (the kernel does not check them, so they are checked here: an empty group and a row outside
    x are refused).  -> (mean64 [groups, d] float64, mean32 [groups, d rounded up to 4] float32 with zero padding, or None)."""
    n, ldx = pitched(x, "backend_group_means: x")
    csr = "backend_group_means: offsets must be a 1-D integer array [groups + 1] that starts at 0"
    offsets = host_ints(offsets, min_size=2, msg=csr)
    if offsets[0] != 0:
        raise ValueError(csr)
    counts = np.diff(offsets.astype(np.int64))
    if counts.min() <= 0:
        raise ValueError("backend_group_means: group %d is empty" % int(np.argmax(counts <= 0)))
    rows = host_ints(rows, "backend_group_means: rows", min_size=1, lo=0, hi=n)
    if rows.size != int(offsets[-1]):
        raise ValueError("backend_group_means: offsets end at %d, rows holds %d indices" % (int(offsets[-1]), rows.size))
    groups = offsets.size - 1
    off_d, rows_d = upload(offsets, np.int64, x.device), upload(rows, np.int32, x.device)
    mean64 = torch.empty((groups, int(d)), dtype=torch.float64, device=x.device)
    mean32 = torch.empty((groups, pitch4(int(d))), dtype=torch.float32, device=x.device) if want32 else None
    _lib.call("xv_backend_group_means", _s(), _p(x), n, ldx, int(d), _p(off_d), _p(rows_d), groups, C.c_int64(rows.size), _p(mean64), _p(mean32),
              mean32.shape[1] if want32 else 0)
    return mean64, mean32


def backend_center(x, d=None, mean=None, out=None):
    """Rows of x [rows, >= d] minus mean [d] (None: a copy) on a zero-padded pitch (xv_backend_center); out as in score_prepare."""
    return _centered("backend_center", "xv_backend_center", x, d, mean, out)


def backend_scatter_workspace_bytes(n, d):
    return int(_lib.load().xv_backend_scatter_workspace_bytes(int(n), int(d)))


def backend_scatter(x, d=None, mean=None, ws_bytes=None):
    """[d, d] float64 = sum over the rows of x [n, >= d] of v v^T, v = x[r][:d] - mean (xv_backend_scatter).  ws_bytes: size of the
    workspace handed to the call (default: what xv_backend_scatter_workspace_bytes asks for; fewer is refused by the library)."""
    n, ldx = pitched(x, "backend_scatter: x")
    d = x.shape[1] if d is None else int(d)
    if mean is not None:
        f32_values(mean, d, "backend_scatter: mean")
    if ws_bytes is None:
        ws_bytes = backend_scatter_workspace_bytes(n, d)
    ws = torch.empty(max(int(ws_bytes) // 4, 1), dtype=torch.float32, device=x.device)
    c64 = torch.empty((max(d, 1), max(d, 1)), dtype=torch.float64, device=x.device)
    _lib.call("xv_backend_scatter", _s(), _p(x), n, d, ldx, _p(mean), _p(c64), _p(ws), C.c_size_t(int(ws_bytes)))
    return c64


def backend_plda_normalize(u, d, psi, n_utts=None, out=None):
    """u[r][:d] * sqrt(d / sum_c u_c^2 / (psi_c + 1 / n_utts[r])) (xv_backend_plda_normalize).  psi: device float32 [d]; n_utts: HOST
    integer array [rows] (None: 1 everywhere), checked positive here.  out: the [rows, pitch] tensor to write, u itself for in place;
    default a new tensor on the pitch d rounded up to 4.  Padding columns come back zero."""
    rows, ldu = pitched(u, "backend_plda_normalize: u")
    d = int(d)
    f32_values(psi, d, "backend_plda_normalize: psi")
    if out is None:
        out = torch.empty((rows, pitch4(max(d, 1))), dtype=torch.float32, device=u.device)
    _, ldo = pitched(out, "backend_plda_normalize: out", whole=True)
    n_d = None
    if n_utts is not None:
        n_utts = host_ints(n_utts, "backend_plda_normalize: n_utts", min_size=1, lo=1, hi=1 << 31)
        if n_utts.size != rows:
            raise ValueError("backend_plda_normalize: n_utts must hold one count per row (%d, got %d)" % (rows, n_utts.size))
        n_d = upload(n_utts, np.int32, u.device)
    _lib.call("xv_backend_plda_normalize", _s(), _p(u), rows, d, ldu, _p(psi), _p(n_d), _p(out), ldo)
    return out


def backend_plda_trials(e, t, d, ei, ti, nidx, coef, g, k0):
    """PLDA log-likelihood ratios of trials (xv_backend_plda_trials): enrol row ei[j] of e against test row ti[j] of t, both transformed
    and normalised.  coef: device float32 [n_distinct, 2, ldc]; g: [>= d]; k0: [n_distinct]; nidx: HOST integer array [enrol rows] into the
    table.  ei, ti, nidx are checked here, before the upload: the kernel does not check indices."""
    ne, lde = pitched(e, "backend_plda_trials: e")
    nt, ldt = pitched(t, "backend_plda_trials: t")
    d = int(d)
    nq, ldc = _plda_tables("backend_plda_trials", coef, g, k0, d)
    ei = host_ints(ei, "backend_plda_trials: ei", min_size=1, lo=0, hi=ne)
    ti = host_ints(ti, "backend_plda_trials: ti", min_size=1, lo=0, hi=nt)
    nidx = host_ints(nidx, "backend_plda_trials: nidx", min_size=1, lo=0, hi=nq)
    if ei.shape != ti.shape or nidx.size != ne:
        raise ValueError("backend_plda_trials: ei and ti must be of one length, nidx one entry per enrol row")
    ei_d, ti_d, nidx_d = (upload(a, np.int32, e.device) for a in (ei, ti, nidx))
    out = torch.empty(ei.size, dtype=torch.float32, device=e.device)
    _lib.call("xv_backend_plda_trials", _s(), _p(e), lde, ne, _p(t), ldt, nt, d, _p(ei_d), _p(ti_d), C.c_int64(ei.size), _p(nidx_d), _p(coef), ldc,
              nq, _p(g), _p(k0), _p(out))
    return out


def _plda_tables(name, coef, g, k0, d):      # the checks plda_trials and plda_cohort_stats share: -> (n_distinct, pitch of coef)
    if coef.dim() != 3 or coef.shape[1] != 2 or coef.dtype != torch.float32 or not coef.is_contiguous() or coef.shape[2] < d:
        raise ValueError("%s: coef must be a contiguous float32 [n_distinct, 2, >= d] tensor" % name)
    nq = coef.shape[0]
    if g.dtype != torch.float32 or g.numel() < d or not g.is_contiguous() or k0.dtype != torch.float32 or k0.numel() != nq or not k0.is_contiguous():
        raise ValueError("%s: g must hold >= d and k0 n_distinct contiguous float32 values" % name)
    return nq, coef.shape[2]


def backend_plda_cohort_workspace_bytes(rows, n_cohort, d, n_distinct):
    return int(_lib.load().xv_backend_plda_cohort_workspace_bytes(int(rows), int(n_cohort), int(d), int(n_distinct)))


def backend_plda_cohort_stats(x, cohort, d, nidx, coef, g, k0, top_k, ws_bytes=None):
    """[rows, 2] = (mean, biased deviation) of each row's min(top_k, n_cohort) largest PLDA log-likelihood ratios against the cohort rows
    (xv_backend_plda_cohort_stats).  x: PLDA-normalised rows in the model role (backend_plda_normalize with their utterance counts), cohort:
    rows normalised with one utterance; both on a zero-padded pitch that is a multiple of 4.  coef, g, k0: plda_coefficients' tables on the
    device; nidx: HOST integer array [rows] into them (None: entry 0 for every row), checked here before the upload.  ws_bytes: size of
    the workspace (default: the whole call in one round); fewer bytes run the rows in tiles."""
    rows, ldx = pitched(x, "backend_plda_cohort_stats: x")
    n_cohort, ldc = pitched(cohort, "backend_plda_cohort_stats: cohort")
    d = int(d)
    nq, ldk = _plda_tables("backend_plda_cohort_stats", coef, g, k0, d)
    nidx_d = None
    if nidx is not None:
        nidx = host_ints(nidx, "backend_plda_cohort_stats: nidx", min_size=1, lo=0, hi=nq)
        if nidx.size != rows:
            raise ValueError("backend_plda_cohort_stats: nidx must hold one entry per row (%d, got %d)" % (rows, nidx.size))
        nidx_d = upload(nidx, np.int32, x.device)
    if ws_bytes is None:
        ws_bytes = backend_plda_cohort_workspace_bytes(rows, n_cohort, d, nq)
    ws = torch.empty(max(int(ws_bytes) // 4, 1), dtype=torch.float32, device=x.device)
    stats = torch.empty((rows, 2), dtype=torch.float32, device=x.device)
    _lib.call("xv_backend_plda_cohort_stats", _s(), _p(x), ldx, rows, _p(nidx_d), _p(cohort), ldc, n_cohort, d, _p(coef), ldk, nq, _p(g), _p(k0),
              int(top_k), _p(stats), _p(ws), C.c_size_t(int(ws_bytes)))
    return stats


def score_normalize(scores, ei, ti, e_stats, t_stats, out=None):
    """AS-norm of scores that are on the device already (xv_score_normalize): out[j] = 0.5 * ((s - mu_e) / sigma_e + (s - mu_t) / sigma_t),
    s = scores[j], the statistics those of rows ei[j] of e_stats [ne, 2] and ti[j] of t_stats [nt, 2] - score_trials' expression, bit for
    bit.  ei, ti: HOST integer arrays, checked here before the upload.  out: the tensor to write (scores itself: in place); default new."""
    if scores.dim() != 1 or scores.dtype != torch.float32 or not scores.is_contiguous() or scores.numel() == 0:
        raise ValueError("score_normalize: scores must be a non-empty contiguous 1-D float32 tensor")
    for st, name in ((e_stats, "e_stats"), (t_stats, "t_stats")):
        if st is None or st.dtype != torch.float32 or st.dim() != 2 or st.shape[1] != 2 or not st.is_contiguous() or st.shape[0] == 0:
            raise ValueError("score_normalize: %s must be a contiguous float32 [n, 2] tensor" % name)
    m = scores.numel()
    ei = host_ints(ei, "score_normalize: ei", n=m, lo=0, hi=e_stats.shape[0])
    ti = host_ints(ti, "score_normalize: ti", n=m, lo=0, hi=t_stats.shape[0])
    if out is None:
        out = torch.empty(m, dtype=torch.float32, device=scores.device)
    elif out.dtype != torch.float32 or out.dim() != 1 or out.numel() != m or not out.is_contiguous():
        raise ValueError("score_normalize: out must be a contiguous 1-D float32 tensor of the scores' length")
    ei_d, ti_d = upload(ei, np.int32, scores.device), upload(ti, np.int32, scores.device)
    _lib.call("xv_score_normalize", _s(), _p(scores), _p(ei_d), _p(ti_d), C.c_int64(m), _p(e_stats), _p(t_stats), _p(out))
    return out


def _dense_out(name, out, n, device):      # the [n, n] matrix a dense op writes: a new one on the pitch n rounded up to 4, or the caller's view
    if out is None:
        return torch.empty((n, pitch4(n)), dtype=torch.float32, device=device)[:, :n]
    rows, ldo = pitched(out, "%s: out" % name)
    if tuple(out.shape) != (n, n) or out.device != device:
        raise ValueError("%s: out must be a float32 [%d, %d] view on the rows' device (its pitch is free)" % (name, n, n))
    return out


def score_dense(x, d, out=None):
    """out[i][j] = x[i][:d] . x[j][:d] for every pair of the prepared rows x (xv_score_dense: score_cohort_stats' GEMM, the rows as their
    own cohort).  out: a float32 [n, n] view of any pitch - into a packed buffer of many recordings, say; default a new matrix.  The two
    triangles are not promised to hold the same bits."""
    n, ldx = pitched(x, "score_dense: x")
    out = _dense_out("score_dense", out, n, x.device)
    _lib.call("xv_score_dense", _s(), _p(x), ldx, n, int(d), _p(out), pitched(out, "score_dense: out")[1])
    return out


def backend_plda_dense_workspace_bytes(n, d):
    return int(_lib.load().xv_backend_plda_dense_workspace_bytes(int(n), int(d)))


def backend_plda_dense(x, d, coef, g, k0, out=None):
    """out[r][j] = the one-utterance PLDA log-likelihood ratio of rows r and j of x, PLDA-normalised with one utterance each
    (xv_backend_plda_dense).  coef, g, k0: plda_coefficients' tables of the single count 1 on the device.  out as in score_dense."""
    n, ldx = pitched(x, "backend_plda_dense: x")
    d = int(d)
    nq, ldk = _plda_tables("backend_plda_dense", coef, g, k0, d)
    if nq != 1:
        raise ValueError("backend_plda_dense: the tables must hold the single entry of one utterance (got %d entries)" % nq)
    out = _dense_out("backend_plda_dense", out, n, x.device)
    ws_bytes = backend_plda_dense_workspace_bytes(n, d)
    ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=x.device)
    _lib.call("xv_backend_plda_dense", _s(), _p(x), ldx, n, d, _p(coef), ldk, _p(g), _p(k0), _p(out), pitched(out, "backend_plda_dense: out")[1],
              _p(ws), C.c_size_t(ws_bytes))
    return out


AHC_MAX_N = 2048      # the rows of one recording xv_ahc_cluster takes


def ahc_workspace_bytes(n):
    """Bytes of scratch xv_ahc_cluster needs for recordings of n[i] rows (a host integer array): every recording's n x n matrix."""
    n = np.asarray(n, dtype=np.int64)
    return int(_lib.load().xv_ahc_workspace_bytes(C.c_int64(int((n * n).sum()))))


def ahc_cluster(scores, mat_offsets, n, ld=None, threshold=0.0, targets=None):
    """Average-linkage agglomerative clustering of b score matrices in one call (xv_ahc_cluster; include/xvector_hip.h states the arithmetic,
    tests/ahc_ref.py restates it).  scores: a contiguous 1-D float32 device buffer; recording i's matrix [n[i], ld[i]] starts at float
    mat_offsets[i] and only its upper triangle is read.  targets[i] = 0 (None: all 0): merge while the best average score is >= threshold;
    t >= 1: merge down to t clusters, whatever the scores.  mat_offsets, n, ld (None: n), targets: HOST integer arrays, checked here before
    the upload - the kernel trusts them.  -> (labels int32 [sum n], merges int32 [sum (n - 1), 2], merge_values float32 [sum (n - 1)],
    n_merges int32 [b]), device tensors; recording i's labels start at the exclusive prefix of n, its merge log at that of n - 1 and holds
    n_merges[i] entries.  A NaN score is undefined."""
    if scores.dtype != torch.float32 or scores.dim() != 1 or not scores.is_contiguous() or scores.numel() == 0:
        raise ValueError("ahc_cluster: scores must be a non-empty contiguous 1-D float32 tensor")
    n = host_ints(n, "ahc_cluster: n", min_size=1)
    b = n.size
    if n.min() < 1:
        raise ValueError("ahc_cluster: recording %d has no row (n = %d)" % (int(np.argmax(n < 1)), int(n.min())))
    if n.max() > AHC_MAX_N:
        raise ValueError("ahc_cluster: recording %d has %d rows, the cap is %d" % (int(np.argmax(n > AHC_MAX_N)), int(n.max()), AHC_MAX_N))
    ld = n if ld is None else host_ints(ld, "ahc_cluster: ld", n=b)
    if (ld < n).any():
        raise ValueError("ahc_cluster: recording %d: the pitch %d is below its %d rows" % (int(np.argmax(ld < n)), int(ld[np.argmax(ld < n)]), int(n[np.argmax(ld < n)])))
    targets = np.zeros(b, np.int32) if targets is None else host_ints(targets, "ahc_cluster: targets", n=b)
    if (targets < 0).any() or (targets > n).any():
        i = int(np.argmax((targets < 0) | (targets > n)))
        raise ValueError("ahc_cluster: recording %d: target %d outside 0 .. %d" % (i, int(targets[i]), int(n[i])))
    mat_offsets = host_ints(mat_offsets, "ahc_cluster: mat_offsets", n=b, dtype=np.int64)
    n64, ld64 = n.astype(np.int64), ld.astype(np.int64)
    spans_inside(mat_offsets, (n64 - 1) * ld64 + n64, scores.numel(), "ahc_cluster: a matrix lies outside the %d floats of scores" % scores.numel())
    dev = scores.device
    total, sum_n2 = int(n64.sum()), int((n64 * n64).sum())
    labels = torch.empty(total, dtype=torch.int32, device=dev)
    merges = torch.empty((max(total - b, 1), 2), dtype=torch.int32, device=dev)
    values = torch.empty(max(total - b, 1), dtype=torch.float32, device=dev)
    n_merges = torch.empty(b, dtype=torch.int32, device=dev)
    ws_bytes = ahc_workspace_bytes(n)
    ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=dev)
    off_d, n_d, ld_d, t_d = upload(mat_offsets, np.int64, dev), upload(n, np.int32, dev), upload(ld, np.int32, dev), upload(targets, np.int32, dev)
    _lib.call("xv_ahc_cluster", _s(), _p(scores), C.c_int64(scores.numel()), _p(off_d), _p(n_d), _p(ld_d), _p(t_d), b, int(n.max()), C.c_int64(total),
              C.c_int64(sum_n2), C.c_float(float(threshold)), _p(labels), _p(merges), _p(values), _p(n_merges), _p(ws), C.c_size_t(ws_bytes))
    return labels, merges[:total - b], values[:total - b], n_merges


AHC_MAX_POINTS = 32768      # the rows of one recording the two-pass clustering takes (xv_ahc_cluster_sums; the sizes of a seed together)


def _ahc_matrices(name, scores, mat_offsets, n, ld, cap):
    """The host checks ahc_cluster makes of its matrices, for the ops of the two-pass clustering.  -> (n, ld, mat_offsets) as host arrays."""
    if scores.dtype != torch.float32 or scores.dim() != 1 or not scores.is_contiguous() or scores.numel() == 0:
        raise ValueError("%s: scores must be a non-empty contiguous 1-D float32 tensor" % name)
    n = host_ints(n, name + ": n", min_size=1)
    b = n.size
    if n.min() < 1:
        raise ValueError("%s: recording %d has no row (n = %d)" % (name, int(np.argmax(n < 1)), int(n.min())))
    if n.max() > cap:
        raise ValueError("%s: recording %d has %d rows, the cap is %d" % (name, int(np.argmax(n > cap)), int(n.max()), cap))
    ld = n if ld is None else host_ints(ld, name + ": ld", n=b)
    if (ld < n).any():
        i = int(np.argmax(ld < n))
        raise ValueError("%s: recording %d: the pitch %d is below its %d rows" % (name, i, int(ld[i]), int(n[i])))
    mat_offsets = host_ints(mat_offsets, name + ": mat_offsets", n=b, dtype=np.int64)
    n64, ld64 = n.astype(np.int64), ld.astype(np.int64)
    spans_inside(mat_offsets, (n64 - 1) * ld64 + n64, scores.numel(), "%s: a matrix lies outside the %d floats of scores" % (name, scores.numel()))
    return n64, ld64, mat_offsets


def ahc_cluster_from(scores, mat_offsets, n, ld=None, floors=None, threshold=float("-inf"), seed=None, sizes=None):
    """The clusterer with a floor (xv_ahc_cluster_from; tests/ahc2_ref.py restates it): recording i merges while it has more than floors[i]
    clusters (1 .. n[i]; None: 1) AND the best average score is >= threshold (-inf: down to the floor).  Two starts.  From scores (seed
    None): scores, mat_offsets, n, ld as for ahc_cluster - a sub-block of a matrix is a matrix at an offset on that matrix's pitch.
    Seeded: seed is a contiguous 1-D float32 device tensor that holds recording i's T [n[i], n[i]] (symmetric, pitch n[i]) at the exclusive
    prefix of n^2 - it is the clusterer's scratch and is MODIFIED -, sizes a HOST integer array [sum n], each >= 1, a recording's together at
    most 32768 (ahc_cluster_sums gives both); scores, mat_offsets and ld must be None.  -> ahc_cluster's four outputs."""
    name = "ahc_cluster_from"
    if seed is None:
        if sizes is not None:
            raise ValueError("%s: sizes belong to a seeded start (seed is None)" % name)
        n, ld, mat_offsets = _ahc_matrices(name, scores, mat_offsets, n, ld, AHC_MAX_N)
        dev = scores.device
    else:
        if scores is not None or mat_offsets is not None or ld is not None:
            raise ValueError("%s: a seeded start reads no scores (scores, mat_offsets and ld must be None)" % name)
        n = host_ints(n, name + ": n", min_size=1, dtype=np.int64)
        if n.min() < 1 or n.max() > AHC_MAX_N:
            i = int(np.argmax((n < 1) | (n > AHC_MAX_N)))
            raise ValueError("%s: recording %d has %d clusters, 1 .. %d are taken" % (name, i, int(n[i]), AHC_MAX_N))
        if seed.dtype != torch.float32 or seed.dim() != 1 or not seed.is_contiguous() or seed.numel() < int((n * n).sum()):
            raise ValueError("%s: seed must be a contiguous 1-D float32 tensor of at least %d floats" % (name, int((n * n).sum())))
        sizes = host_ints(sizes if sizes is not None else [], name + ": sizes", n=int(n.sum()))
        members = np.add.reduceat(np.maximum(sizes, 0).astype(np.int64), exclusive_offsets(n))
        wrong = (np.minimum.reduceat(sizes, exclusive_offsets(n)) < 1) | (members > AHC_MAX_POINTS)
        if wrong.any():
            raise ValueError("%s: recording %d: the sizes must be positive and add up to at most %d" % (name, int(np.argmax(wrong)), AHC_MAX_POINTS))
        dev = seed.device
    b = n.size
    floors = np.ones(b, np.int32) if floors is None else host_ints(floors, name + ": floors", n=b)
    if (floors < 1).any() or (floors > n).any():
        i = int(np.argmax((floors < 1) | (floors > n)))
        raise ValueError("%s: recording %d: floor %d outside 1 .. %d" % (name, i, int(floors[i]), int(n[i])))
    threshold = float(threshold)
    if threshold != threshold:
        raise ValueError("%s: the threshold is NaN" % name)
    total, sum_n2 = int(n.sum()), int((n * n).sum())
    labels = torch.empty(total, dtype=torch.int32, device=dev)
    merges = torch.empty((max(total - b, 1), 2), dtype=torch.int32, device=dev)
    values = torch.empty(max(total - b, 1), dtype=torch.float32, device=dev)
    n_merges = torch.empty(b, dtype=torch.int32, device=dev)
    n_d, f_d = upload(n, np.int32, dev), upload(floors, np.int32, dev)
    if seed is None:
        ws_bytes = int(_lib.load().xv_ahc_cluster_from_workspace_bytes(C.c_int64(sum_n2)))
        ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=dev)
        off_d, ld_d, s_d = upload(mat_offsets, np.int64, dev), upload(ld, np.int32, dev), None
    else:
        ws, ws_bytes, off_d, ld_d, s_d = seed, seed.numel() * 4, None, None, upload(sizes, np.int32, dev)
    _lib.call("xv_ahc_cluster_from", _s(), _p(scores), C.c_int64(scores.numel() if scores is not None else 0), _p(off_d), _p(n_d), _p(ld_d), _p(f_d),
              _p(s_d), int(seed is not None), b, int(n.max()), C.c_int64(total), C.c_int64(sum_n2), C.c_float(threshold), _p(labels), _p(merges),
              _p(values), _p(n_merges), _p(ws), C.c_size_t(ws_bytes))
    return labels, merges[:total - b], values[:total - b], n_merges


def ahc_member_lists(labels, n):
    """Clusters as the member lists ahc_cluster_sums takes, from HOST labels [sum n] (recording i's n[i] back to back, numbered 0, 1, ... in
    the order of their smallest members, as the clusterer numbers them).  -> (members int32 [sum n], starts int32 [sum (c + 1)], c int64 [b])."""
    n = host_ints(n, "ahc_member_lists: n", min_size=1, dtype=np.int64)
    labels = host_ints(labels, "ahc_member_lists: labels", n=int(n.sum()))
    members, starts, c = [], [], []
    for lo, hi in zip(exclusive_offsets(n), np.cumsum(n)):
        lab = labels[lo:hi]
        uniq, first = np.unique(lab, return_index=True)
        if lab.size == 0 or uniq[0] != 0 or uniq[-1] != uniq.size - 1 or (np.diff(first) <= 0).any():
            raise ValueError("ahc_member_lists: a recording's labels must be 0, 1, ... in the order of the clusters' smallest members")
        members.append(np.argsort(lab, kind="stable").astype(np.int32))
        starts.append(np.concatenate([[0], np.cumsum(np.bincount(lab))]).astype(np.int32))
        c.append(uniq.size)
    return np.concatenate(members), np.concatenate(starts), np.asarray(c, np.int64)


def ahc_cluster_sums_workspace_bytes(n, c):
    """Bytes of scratch xv_ahc_cluster_sums needs for recordings of n[i] rows in c[i] clusters (host integer arrays of one length)."""
    n, c = np.asarray(n, dtype=np.int64), np.asarray(c, dtype=np.int64)
    return int(_lib.load().xv_ahc_cluster_sums_workspace_bytes(int(n.size), C.c_int64(int((n * c).sum()))))


def ahc_cluster_sums(scores, mat_offsets, n, ld, members, starts, c):
    """The seed of a second clustering pass (xv_ahc_cluster_sums; include/xvector_hip.h states the order of every sum, tests/ahc2_ref.py
    restates it): T[A][B] = the sum of the scores between the members of clusters A and B of each of b recordings, from the upper triangles
    of their matrices (scores, mat_offsets, n <= 32768, ld as for ahc_cluster).  members, starts, c: HOST integer arrays as ahc_member_lists
    gives them - recording i's rows cluster by cluster, clusters ascending by smallest member, members ascending; c[i] <= 2048 - checked
    here before the upload.  -> (seed float32 [sum c^2], sizes int32 [sum c]), device tensors: what ahc_cluster_from takes for a seeded start."""
    name = "ahc_cluster_sums"
    n, ld, mat_offsets = _ahc_matrices(name, scores, mat_offsets, n, ld, AHC_MAX_POINTS)
    b = n.size
    c = host_ints(c, name + ": c", n=b, dtype=np.int64)
    if (c < 1).any() or (c > np.minimum(n, AHC_MAX_N)).any():
        i = int(np.argmax((c < 1) | (c > np.minimum(n, AHC_MAX_N))))
        raise ValueError("%s: recording %d has %d clusters, 1 .. %d are taken" % (name, i, int(c[i]), int(min(n[i], AHC_MAX_N))))
    members = host_ints(members, name + ": members", n=int(n.sum()))
    starts = host_ints(starts, name + ": starts", n=int(c.sum()) + b)
    for i, (m0, s0) in enumerate(zip(exclusive_offsets(n), exclusive_offsets(c + 1))):
        st, mem = starts[s0:s0 + c[i] + 1], members[m0:m0 + n[i]]
        if st[0] != 0 or st[-1] != n[i] or (np.diff(st) <= 0).any():
            raise ValueError("%s: recording %d: starts must ascend from 0 to its %d rows" % (name, i, int(n[i])))
        inner = np.ones(mem.size, bool)
        inner[st[:-1]] = False      # (the first member of a cluster need not be above the last of the cluster before)
        if not np.array_equal(np.sort(mem), np.arange(n[i])) or (np.diff(mem)[inner[1:]] <= 0).any() or (np.diff(mem[st[:-1]]) <= 0).any():
            raise ValueError("%s: recording %d: members must hold every row once, clusters ascending by their smallest member, a cluster's "
                             "members ascending" % (name, i))
    dev = scores.device
    seed = torch.empty(int((c * c).sum()), dtype=torch.float32, device=dev)
    sizes = torch.empty(int(c.sum()), dtype=torch.int32, device=dev)
    status = torch.empty(b, dtype=torch.int32, device=dev)
    ws_bytes = ahc_cluster_sums_workspace_bytes(n, c)
    ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=dev)
    off_d, n_d, ld_d, c_d = upload(mat_offsets, np.int64, dev), upload(n, np.int32, dev), upload(ld, np.int32, dev), upload(c, np.int32, dev)
    mem_d, st_d = upload(members, np.int32, dev), upload(starts, np.int32, dev)
    _lib.call("xv_ahc_cluster_sums", _s(), _p(scores), C.c_int64(scores.numel()), _p(off_d), _p(n_d), _p(ld_d), _p(c_d),
              _p(mem_d), _p(st_d), b, int(n.max()), int(c.max()), C.c_int64(int(n.sum())), C.c_int64(int(c.sum())),
              C.c_int64(int((c * c).sum())), C.c_int64(int((n * c).sum())), _p(seed), _p(sizes), _p(status), _p(ws), C.c_size_t(ws_bytes))
    if int(status.min()) != 0:
        raise RuntimeError("%s: xv_ahc_cluster_sums skipped recording %d" % (name, int(torch.argmin(status))))
    return seed, sizes


def ahc_subsets(n, first_pass_max_points):
    """The contiguous subsets of the first pass for a recording of n rows: ceil(n / first_pass_max_points) of them, ceil(n / that number)
    rows each, the last one shorter.  -> the boundaries, int64 [subsets + 1], from 0 to n."""
    n, cap = int(n), int(first_pass_max_points)
    subsets = -(-n // cap)
    size = -(-n // subsets)
    return np.minimum(np.arange(subsets + 1, dtype=np.int64) * size, n)


def ahc_cluster_two_pass(scores, mat_offsets, n, ld=None, threshold=0.0, targets=None, first_pass_max_points=AHC_MAX_N):
    """Two-pass clustering of recordings of up to 32768 rows (Kaldi's AgglomerativeClusterer::ClusterTwoPass, recalled and restated - not
    compared with a Kaldi run, max_spk_fraction left out; tests/ahc2_ref.py restates this driver).  scores, mat_offsets, n, ld as for
    ahc_cluster.  targets None: every recording merges while the best average score is >= threshold; else targets[i] >= 1 clusters for
    every recording (a call has one stop rule).  A recording of more than first_pass_max_points (2 .. 2048) rows is cut into ahc_subsets;
    one ahc_cluster_from call clusters every subset of every recording down to min(its rows, 10 x max(target, 1)) clusters (or until the
    threshold stops it); ahc_cluster_sums adds up the scores between the surviving clusters, and one seeded ahc_cluster_from call merges
    them down to the target (threshold -inf) or the threshold (floor 1).  A row's label is the second-pass label of its first-pass
    cluster; final clusters are numbered by their smallest members.  A shorter recording is one subset that the first pass clusters to the
    end; its second pass merges nothing.  The first pass's labels come back to the host between the passes (one synchronisation).
    -> (labels int32 [sum n] on the device, first, second, subsets): first / second = (merges, merge_values, n_merges) of the two
    ahc_cluster_from calls - the first per subset in order, in the subset's row numbers; the second per recording, in first-pass cluster
    numbers -, subsets = [ahc_subsets(n[i])] per recording."""
    name = "ahc_cluster_two_pass"
    n, ld, mat_offsets = _ahc_matrices(name, scores, mat_offsets, n, ld, AHC_MAX_POINTS)
    b, cap = n.size, int(first_pass_max_points)
    if not 2 <= cap <= AHC_MAX_N:
        raise ValueError("%s: first_pass_max_points must lie in 2 .. %d (got %d)" % (name, AHC_MAX_N, cap))
    if targets is None:
        targets = np.zeros(b, np.int64)
    else:
        targets = host_ints(targets, name + ": targets", n=b, dtype=np.int64)
        if (targets < 1).any() or (targets > n).any():
            i = int(np.argmax((targets < 1) | (targets > n)))
            raise ValueError("%s: recording %d: target %d outside 1 .. %d (None: the threshold, for every recording)" % (name, i, int(targets[i]), int(n[i])))
        threshold = float("-inf")
    ends = np.maximum(targets, 1)      # where a recording's merging may end at the latest
    subsets = [ahc_subsets(r, cap) for r in n]
    sub_off, sub_n, sub_ld, sub_floor = [], [], [], []
    for i, bounds in enumerate(subsets):
        rows = np.diff(bounds)
        sub_off.append(mat_offsets[i] + bounds[:-1] * (ld[i] + 1))
        sub_n.append(rows)
        sub_ld.append(np.full(rows.size, ld[i]))
        sub_floor.append(np.minimum(rows, 10 * ends[i]) if rows.size > 1 else ends[i:i + 1])
    sub_n = np.concatenate(sub_n)
    labels1, merges1, values1, n_merges1 = ahc_cluster_from(scores, np.concatenate(sub_off), sub_n, np.concatenate(sub_ld), floors=np.concatenate(sub_floor),
                                                            threshold=threshold)
    local = labels1.cpu().numpy().astype(np.int64)
    if int(n_merges1.min()) < 0:
        raise RuntimeError("%s: xv_ahc_cluster_from skipped subset %d" % (name, int(torch.argmin(n_merges1))))
    # a recording's first-pass clusters, numbered through its subsets: ascending by smallest member, since the subsets are contiguous
    clusters, c, at = np.empty(int(n.sum()), np.int64), np.zeros(b, np.int64), 0
    for i, bounds in enumerate(subsets):
        for rows in np.diff(bounds):
            clusters[at:at + rows] = c[i] + local[at:at + rows]
            c[i] += local[at:at + rows].max() + 1
            at += rows
        if c[i] > AHC_MAX_N:
            what = "the first pass leaves %d clusters, the second pass takes %d (lower the threshold or first_pass_max_points)" % (int(c[i]), AHC_MAX_N)
            error = ValueError("%s: recording %d: %s" % (name, i, what))
            error.recording, error.what = i, what      # (for a caller that knows the recording by name)
            raise error
    members, starts, _ = ahc_member_lists(clusters, n)
    seed, _ = ahc_cluster_sums(scores, mat_offsets, n, ld, members, starts, c)
    sizes = np.concatenate([np.bincount(clusters[lo:hi]) for lo, hi in zip(exclusive_offsets(n), np.cumsum(n))])
    floors2 = np.where(n > cap, ends, c)      # (a short recording is done)
    labels2, merges2, values2, n_merges2 = ahc_cluster_from(None, None, c, floors=floors2, threshold=threshold, seed=seed, sizes=sizes)
    if int(n_merges2.min()) < 0:
        raise RuntimeError("%s: xv_ahc_cluster_from skipped recording %d in the second pass" % (name, int(torch.argmin(n_merges2))))
    index = upload(clusters + np.repeat(exclusive_offsets(c), n), np.int64, scores.device)
    return labels2[index], (merges1, values1, n_merges1), (merges2, values2, n_merges2), subsets


VBX_MAX_SPEAKERS = 32     # the speakers (HMM states) of one recording xv_vbx takes
VBX_MAX_DIM = 256          # ... the dimensions of its rows
VBX_MAX_ITERS = 64         # ... and the iterations of one call


def vbx_workspace_bytes(t, s, d):
    """Bytes of scratch xv_vbx needs for recordings of t[i] rows and s[i] speakers (host integer arrays of one length) in d dimensions."""
    t, s = np.asarray(t, dtype=np.int64), np.asarray(s, dtype=np.int64)
    return int(_lib.load().xv_vbx_workspace_bytes(C.c_int64(int(t.sum())), C.c_int64(int((t * s).sum())), C.c_int64(int(s.sum())), int(d)))


def vbx(x, x_offsets, t, d, phi, gamma, pi, s, ld=None, loop_prob=0.99, fa=0.3, fb=17.0, max_iters=20, epsilon=1e-4):
    """VB-HMM clustering (VBx) of b recordings in one call (xv_vbx; include/xvector_hip.h states the arithmetic, tests/vbx_ref.py restates
    it).  x: a contiguous 1-D float32 device buffer; recording i's rows [t[i], ld[i]] (ld None: d) start at float x_offsets[i]: vectors in
    the PLDA space with within-class covariance I and between-class covariance diag(phi) (BackendScorer.plda_space).  phi: float32 [d]
    on the device.  gamma: the initial responsibilities, recording i's [t[i], s[i]] back to back in one 1-D float32 device tensor; pi: the
    initial priors, recording i's [s[i]] back to back.  x_offsets, t, ld, s: HOST integer arrays, checked here before the upload - the
    kernel trusts them.  epsilon: the smallest gain of the ELBO that keeps iterating (-inf: always max_iters).
    -> (gamma, pi, elbo float64 [b, max_iters] - NaN behind the iterations run -, n_iters int32 [b], labels int32 [sum t]), device tensors
    laid out as the inputs; x, phi and the initial gamma and pi are not modified."""
    if x.dtype != torch.float32 or x.dim() != 1 or not x.is_contiguous() or x.numel() == 0:
        raise ValueError("vbx: x must be a non-empty contiguous 1-D float32 tensor")
    d, max_iters = int(d), int(max_iters)
    if not 1 <= d <= VBX_MAX_DIM:
        raise ValueError("vbx: d must lie in 1 .. %d (got %d)" % (VBX_MAX_DIM, d))
    if not 1 <= max_iters <= VBX_MAX_ITERS:
        raise ValueError("vbx: max_iters must lie in 1 .. %d (got %d)" % (VBX_MAX_ITERS, max_iters))
    loop32 = float(np.float32(loop_prob))
    if not 0.0 < loop32 < 1.0:
        raise ValueError("vbx: loop_prob must lie strictly between 0 and 1 as a float32 (got %r)" % (loop_prob,))
    if not (float(np.float32(fa)) > 0.0 and float(np.float32(fb)) > 0.0 and np.isfinite(np.float32(fa)) and np.isfinite(np.float32(fb))):
        raise ValueError("vbx: fa and fb must be positive (got %r, %r)" % (fa, fb))
    if np.isnan(epsilon):
        raise ValueError("vbx: epsilon is not a number")
    t = host_ints(t, "vbx: t", min_size=1)
    b = t.size
    if t.min() < 1:
        raise ValueError("vbx: recording %d has no row (t = %d)" % (int(np.argmax(t < 1)), int(t.min())))
    if t.max() > AHC_MAX_N:
        raise ValueError("vbx: recording %d has %d rows, the cap is %d" % (int(np.argmax(t > AHC_MAX_N)), int(t.max()), AHC_MAX_N))
    s = host_ints(s, "vbx: s", n=b)
    if s.min() < 1:
        raise ValueError("vbx: recording %d has no speaker (s = %d)" % (int(np.argmax(s < 1)), int(s.min())))
    if s.max() > VBX_MAX_SPEAKERS:
        raise ValueError("vbx: recording %d has %d speakers, the cap is %d" % (int(np.argmax(s > VBX_MAX_SPEAKERS)), int(s.max()), VBX_MAX_SPEAKERS))
    ld = np.full(b, d, np.int64) if ld is None else host_ints(ld, "vbx: ld", n=b)
    if (ld < d).any():
        raise ValueError("vbx: recording %d: the pitch %d is below the %d dimensions" % (int(np.argmax(ld < d)), int(ld[np.argmax(ld < d)]), d))
    x_offsets = host_ints(x_offsets, "vbx: x_offsets", n=b, dtype=np.int64)
    t64, s64, ld64 = t.astype(np.int64), s.astype(np.int64), ld.astype(np.int64)
    spans_inside(x_offsets, (t64 - 1) * ld64 + d, x.numel(), "vbx: a recording's rows lie outside the %d floats of x" % x.numel())
    total_t, total_ts, total_s = int(t64.sum()), int((t64 * s64).sum()), int(s64.sum())
    f32_values(phi, d, "vbx: phi")
    f32_values(gamma, total_ts, "vbx: gamma (sum of t * s)")
    f32_values(pi, total_s, "vbx: pi (sum of s)")
    dev = x.device
    gamma_out, pi_out = torch.empty_like(gamma), torch.empty_like(pi)
    elbo = torch.full((b, max_iters), float("nan"), dtype=torch.float64, device=dev)
    n_iters = torch.empty(b, dtype=torch.int32, device=dev)
    labels = torch.empty(total_t, dtype=torch.int32, device=dev)
    ws_bytes = vbx_workspace_bytes(t, s, d)
    ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=dev)
    off_d, t_d, ld_d, s_d = upload(x_offsets, np.int64, dev), upload(t, np.int32, dev), upload(ld, np.int32, dev), upload(s, np.int32, dev)
    _lib.call("xv_vbx", _s(), _p(x), C.c_int64(x.numel()), _p(off_d), _p(t_d), _p(ld_d), _p(s_d), b, d, int(t.max()), int(s.max()), C.c_int64(total_t),
              C.c_int64(total_ts), C.c_int64(total_s), _p(phi), _p(gamma), _p(pi), C.c_float(loop32), C.c_float(float(fa)), C.c_float(float(fb)),
              max_iters, C.c_double(float(epsilon)), _p(gamma_out), _p(pi_out), _p(elbo), _p(n_iters), _p(labels), _p(ws), C.c_size_t(ws_bytes))
    return gamma_out, pi_out, elbo, n_iters, labels


PCA_MAX_DIM = 256      # the dimensions of the rows xv_backend_pca_plda takes


def backend_pca_plda_workspace_bytes(b, d):
    """Bytes of scratch xv_backend_pca_plda needs for b recordings in d dimensions."""
    return int(_lib.load().xv_backend_pca_plda_workspace_bytes(int(b), int(d)))


def backend_pca_plda(x, x_offsets, n, d, w, b, mu, target, ld=None):
    """The per-recording PCA of ivector-plda-scoring-dense --target-energy for the recordings of one call (xv_backend_pca_plda;
    include/xvector_hip.h states the arithmetic, tests/pca_plda_ref.py restates it).  x: a contiguous 1-D float32 device buffer; recording
    i's rows [n[i], ld[i]] (ld None: d) start at float x_offsets[i]: centred, LDA-transformed, unit-length vectors.  w, b: float64 [d, d]
    device tensors, the within- and between-class covariances of the PLDA model (misc.backend.plda_covariances); mu: float64 [d], its
    mean.  target: the share of the energy to keep, in (0, 1].  x_offsets, n, ld: HOST integer arrays, checked here before the upload - the
    kernel trusts them.
    -> dict of device tensors, d4 = d rounded up to 4: p int32 [recordings] (0: no PCA for this recording, use the global model; -2 / -3: the
    eigensolver reached its sweep cap / the projected within-class covariance is not positive definite), a float32 [recordings, d4, d4] (the
    first p rows and d columns hold the map, the rest zero), offset, psi, g float32 [recordings, d4], coef float32 [recordings, 2, d4],
    k0 float32 [recordings], s, psi64 float64 [recordings, d], sweeps int32 [recordings, 2].  What the kernel does not write - everything
    but p (and s) of a recording with p <= 0, psi64 behind p - stays NaN (sweeps: -1)."""
    if x.dtype != torch.float32 or x.dim() != 1 or not x.is_contiguous() or x.numel() == 0:
        raise ValueError("backend_pca_plda: x must be a non-empty contiguous 1-D float32 tensor")
    d, target = int(d), float(target)
    if not 1 <= d <= PCA_MAX_DIM:
        raise ValueError("backend_pca_plda: d must lie in 1 .. %d (got %d)" % (PCA_MAX_DIM, d))
    if not 0.0 < target <= 1.0:
        raise ValueError("backend_pca_plda: target must lie in (0, 1] (got %r)" % (target,))
    n = host_ints(n, "backend_pca_plda: n", min_size=1)
    count = n.size
    if n.min() < 1:
        raise ValueError("backend_pca_plda: recording %d has no row (n = %d)" % (int(np.argmax(n < 1)), int(n.min())))
    if n.max() > AHC_MAX_N:
        raise ValueError("backend_pca_plda: recording %d has %d rows, the cap is %d" % (int(np.argmax(n > AHC_MAX_N)), int(n.max()), AHC_MAX_N))
    ld = np.full(count, d, np.int64) if ld is None else host_ints(ld, "backend_pca_plda: ld", n=count)
    if (ld < d).any():
        raise ValueError("backend_pca_plda: recording %d: the pitch %d is below the %d dimensions" % (int(np.argmax(ld < d)), int(ld[np.argmax(ld < d)]), d))
    x_offsets = host_ints(x_offsets, "backend_pca_plda: x_offsets", n=count, dtype=np.int64)
    spans_inside(x_offsets, (n.astype(np.int64) - 1) * ld.astype(np.int64) + d, x.numel(),
                 "backend_pca_plda: a recording's rows lie outside the %d floats of x" % x.numel())
    for t, shape, name in ((w, (d, d), "w"), (b, (d, d), "b"), (mu, (d,), "mu")):
        if t.dtype != torch.float64 or tuple(t.shape) != shape or not t.is_contiguous() or t.device != x.device:
            raise ValueError("backend_pca_plda: %s must be a contiguous float64 %s tensor on the rows' device" % (name, list(shape)))
    dev, d4 = x.device, pitch4(d)
    nan32 = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device=dev)
    out = dict(p=torch.empty(count, dtype=torch.int32, device=dev), a=nan32(count, d4, d4), offset=nan32(count, d4), psi=nan32(count, d4),
               coef=nan32(count, 2, d4), g=nan32(count, d4), k0=nan32(count),
               s=torch.full((count, d), float("nan"), dtype=torch.float64, device=dev),
               psi64=torch.full((count, d), float("nan"), dtype=torch.float64, device=dev),
               sweeps=torch.full((count, 2), -1, dtype=torch.int32, device=dev))
    ws_bytes = backend_pca_plda_workspace_bytes(count, d)
    ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=dev)
    off_d, n_d, ld_d = upload(x_offsets, np.int64, dev), upload(n, np.int32, dev), upload(ld, np.int32, dev)
    _lib.call("xv_backend_pca_plda", _s(), _p(x), C.c_int64(x.numel()), _p(off_d), _p(n_d), _p(ld_d), count, d, int(n.max()), C.c_double(target),
              _p(w), _p(b), _p(mu), _p(out["p"]), _p(out["a"]), _p(out["offset"]), _p(out["psi"]), _p(out["coef"]), _p(out["g"]), _p(out["k0"]),
              _p(out["s"]), _p(out["psi64"]), _p(out["sweeps"]), _p(ws), C.c_size_t(ws_bytes))
    return out
