"""Op-level wrappers of the pipeline stages around the network that take feature matrices or vectors (include/xvector_hip.h): the extraction
front end, the 'CM ' codec, cosine / AS-norm / dense scoring and the LDA / PLDA back end with its cohort statistics; those that take PCM are
in wave_ops.py, those of diarization (clustering, VBx, the per-recording PCA) in diar_ops.py.  ops.py re-exports every public name here: callers write
ops.score_trials.  Their kernels check none of the index arrays they are handed, so much of this is validation (_host.host_ints) in front of one upload."""
import ctypes as C

import numpy as np
import torch

try:
    from ._host import _lib, _p, _s, exclusive_offsets, f32_buffer, f32_values, host_ints, pitch4, pitched, spans_inside, upload
except ImportError:
    from _host import _lib, _p, _s, exclusive_offsets, f32_buffer, f32_values, host_ints, pitch4, pitched, spans_inside, upload


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
    m = f32_buffer(scores, "score_normalize: scores")
    for st, name in ((e_stats, "e_stats"), (t_stats, "t_stats")):
        if st is None or st.dtype != torch.float32 or st.dim() != 2 or st.shape[1] != 2 or not st.is_contiguous() or st.shape[0] == 0:
            raise ValueError("score_normalize: %s must be a contiguous float32 [n, 2] tensor" % name)
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
