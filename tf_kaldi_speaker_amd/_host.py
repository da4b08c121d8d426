"""What the host side of every op has in common: device buffers as ctypes arguments, the checks of host index arrays that the kernels
leave to the caller (index arrays, spans inside a pool of samples, the recordings of a diarization call, where waveform outputs go, the
size of a constant table), pitches, offsets and bounds, and how the drivers in misc/ cut their work into calls and pack it.  ops.py,
wave_ops.py, pipeline_ops.py, diar_ops.py and misc/ build on this module; it imports none of them at load time."""
import ctypes as C

import numpy as np
import torch

try:
    from . import _lib
except ImportError:
    import _lib

DEFAULT_WORKSPACE_BYTES = 1 << 30      # what the drivers in misc/ let one call take, unless told otherwise


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _s():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _f32(shape, like):
    return torch.empty(shape, dtype=torch.float32, device=like.device)


_WS = {}


def workspace(device, nbytes=256 << 20):
    key = (str(device), nbytes)
    if key not in _WS:
        _WS[key] = torch.empty(nbytes // 4, dtype=torch.float32, device=device)
    return _WS[key]


def _ws(t):
    w = workspace(t.device)
    return _p(w), C.c_size_t(w.numel() * 4)


def device_ops(device):
    """(torch, ops, torch.device(device)) for a driver in misc/, in either import style: tf_kaldi_speaker_amd.X, or flat from the package directory."""
    try:
        from . import ops
    except ImportError:
        import ops
    return torch, ops, torch.device(device)


def upload(a, dtype, device):      # a host array as a contiguous device tensor of `dtype` (np.int32 / np.int64 for index arrays)
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(device)


def host_ints(a, what="", n=None, min_size=0, lo=None, hi=None, msg=None, dtype=None):
    """A 1-D host integer array as a NumPy array (of `dtype` when given, else its own) - the kernels check no index, so index arrays pass here before
    their upload.  n: the exact length; min_size: 1 refuses an empty one; lo, hi: values lie in [lo, hi) (IndexError).  `what` starts the messages, `msg` is the first."""
    a = np.asarray(a)
    if a.ndim != 1 or a.dtype.kind not in "iu" or a.size < min_size or (n is not None and a.size != n):
        raise ValueError(msg or "%s must be a %s1-D integer array%s" % (what, "non-empty " if min_size else "", "" if n is None else " of %d" % n))
    if lo is not None and a.size and (a.min() < lo or a.max() >= hi):
        raise IndexError("%s holds a value outside %d .. %d" % (what, lo, hi - 1))
    return a if dtype is None else a.astype(dtype)


def f32_values(t, d, what):
    if t.dtype != torch.float32 or t.numel() != d or not t.is_contiguous():
        raise ValueError("%s must be %d contiguous float32 values" % (what, d))


def pitched(t, what, whole=False):
    """(rows, pitch in floats) of a 2-D float32 device view with contiguous rows; whole: it must be all of a [rows, pitch] buffer (an
    output of the kernels that write the padding columns too)."""
    if t.dim() != 2 or t.dtype != torch.float32 or (t.shape[1] > 1 and t.stride(1) != 1):
        raise ValueError("%s: a 2-D float32 tensor with contiguous rows is expected" % what)
    ld = t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1])
    if whole and t.shape[1] != ld:
        raise ValueError("%s must be the whole [rows, pitch] buffer (its padding columns are written)" % what)
    return t.shape[0], ld


GE2E_MAX_ROWS = 1024        # csrc/xv_triplet.hip TP_MAX_B: the rows the pairwise and GE2E heads take


def ge2e_rows(x, speakers, segments, d, what="ge2e loss"):
    """(rows, pitch) of the embeddings x of a GE2E batch - speakers x segments speaker-major rows of d floats; what the entry points refuse
    of a layout is refused here by name, before anything is allocated for it."""
    b, ldx = pitched(x, "%s: x" % what)
    n, m = int(speakers), int(segments)
    if n < 1 or m < 1:
        raise ValueError("%s: %d speakers x %d segments" % (what, n, m))
    if m == 1:
        raise ValueError("%s: num_segments_per_speaker is 1: a row needs another row of its speaker" % what)
    if b != n * m:
        raise ValueError("%s: %d rows are not %d speakers x %d segments" % (what, b, n, m))
    if b > GE2E_MAX_ROWS:
        raise ValueError("%s: %d rows, 2 .. %d are supported" % (what, b, GE2E_MAX_ROWS))
    if d < 4 or d % 4 or d > x.shape[1]:
        raise ValueError("%s: the embedding dimension %d must be a positive multiple of 4 (x has %d columns)" % (what, d, x.shape[1]))
    return b, ldx


def pcm_samples(t, what):      # the samples of a pool of signals: a contiguous 1-D int16 device tensor, or None (no pool)
    if t is None:
        return 0
    if t.dtype != torch.int16 or t.dim() != 1 or not t.is_contiguous():
        raise ValueError("%s must be a contiguous 1-D int16 tensor" % what)
    return t.numel()


def spans_inside(offsets, lengths, size, msg, min_length=0):
    """Refuses with IndexError(msg) a span offsets[i] .. offsets[i] + lengths[i] (two host integer arrays of one length, host_ints' results)
    that leaves the `size` elements of its pool, one shorter than min_length (1: no empty span), and a table without a span."""
    if offsets.size == 0 or offsets.min() < 0 or lengths.min() < min_length or (offsets.astype(np.int64) + lengths.astype(np.int64)).max() > size:
        raise IndexError(msg)


def f32_buffer(t, what):      # a pool of floats that index arrays point into: a non-empty contiguous 1-D float32 tensor -> its floats
    if t.dtype != torch.float32 or t.dim() != 1 or not t.is_contiguous() or t.numel() == 0:
        raise ValueError("%s must be a non-empty contiguous 1-D float32 tensor" % what)
    return t.numel()


def recordings(name, buf, offsets, n, ld, cap, letter="n", d=None):
    """The recordings of one call of a diarization op, checked - the kernels trust them - and refused in `name`: recording i lies at float
    offsets[i] of the 1-D float32 buffer buf with n[i] rows (1 .. cap; `letter`: the op's name for n) on the pitch ld[i].  d None: a square
    matrix of `scores` at `mat_offsets`, ld None: n; else rows of d floats of `x` at `x_offsets`, ld None: d.  -> (n, ld, offsets) int64."""
    what, at, lies = ("scores", "mat_offsets", "a matrix lies") if d is None else ("x", "x_offsets", "a recording's rows lie")
    floats = f32_buffer(buf, "%s: %s" % (name, what))
    n = host_ints(n, "%s: %s" % (name, letter), min_size=1, dtype=np.int64)
    if n.min() < 1:
        raise ValueError("%s: recording %d has no row (%s = %d)" % (name, int(np.argmax(n < 1)), letter, int(n.min())))
    if n.max() > cap:
        raise ValueError("%s: recording %d has %d rows, the cap is %d" % (name, int(np.argmax(n > cap)), int(n.max()), cap))
    width = n if d is None else np.full(n.size, d, np.int64)      # what a row holds: the least pitch
    ld = width if ld is None else host_ints(ld, name + ": ld", n=n.size, dtype=np.int64)
    if (ld < width).any():
        i = int(np.argmax(ld < width))
        raise ValueError("%s: recording %d: the pitch %d is below %s" % (name, i, int(ld[i]), "its %d rows" % n[i] if d is None else "the %d dimensions" % d))
    offsets = host_ints(offsets, "%s: %s" % (name, at), n=n.size, dtype=np.int64)
    spans_inside(offsets, (n - 1) * ld + width, floats, "%s: %s outside the %d floats of %s" % (name, lies, floats, what))
    return n, ld, offsets


def cluster_outputs(n, device):
    """What a clusterer writes for recordings of n[i] rows, uninitialised: labels [sum n], merges [sum (n - 1), 2], merge_values [sum (n - 1)]
    - one entry at the least - and n_merges [b].  -> (the four tensors to launch with, the four the op returns: the merge log cut to size)."""
    total, b = int(n.sum()), n.size
    shapes = ((total, torch.int32), ((max(total - b, 1), 2), torch.int32), (max(total - b, 1), torch.float32), (b, torch.int32))
    labels, merges, values, n_merges = (torch.empty(shape, dtype=dtype, device=device) for shape, dtype in shapes)
    return (labels, merges, values, n_merges), (labels, merges[:total - b], values[:total - b], n_merges)


def pack_rows(matrices):      # [n_i, ld] device matrices on one pitch -> (x 1-D, offsets, n, ld [b]): one call's recordings; one alone is not copied
    n = np.asarray([m.shape[0] for m in matrices], np.int64)
    x = torch.cat([m.reshape(-1) for m in matrices]) if len(matrices) > 1 else matrices[0].reshape(-1)
    return x, bounds(n)[:-1] * matrices[0].shape[1], n, np.full(n.size, matrices[0].shape[1], np.int64)


def place_outputs(name, n_out, out_offsets, out_pcm, out_f32, device, min_samples=0):
    """Where the ops that write waveforms put them: out_offsets (None: the n_out [b] samples of each back to back), out_pcm (None: a new
    int16 tensor that just holds them, min_samples at the least) and out_f32 (True: a new float32 tensor of out_pcm's size, False: none,
    or such a tensor), checked - the kernels do not - and refused in `name`.  -> (out_pcm, out_offsets int64 [b], out_f32 | None)."""
    out_offsets = host_ints(exclusive_offsets(n_out) if out_offsets is None else out_offsets, name + ": out_offsets", n=n_out.size, dtype=np.int64)
    ends = out_offsets + n_out
    if out_pcm is None:
        out_pcm = torch.empty(max(int(ends.max()), min_samples), dtype=torch.int16, device=device)
    total = pcm_samples(out_pcm, name + ": out_pcm")
    order = np.argsort(out_offsets, kind="stable")
    if out_offsets.min() < 0 or ends.max() > total or (out_offsets[order][1:] < ends[order][:-1]).any():
        raise IndexError("%s: the outputs overlap or lie outside the %d samples of out_pcm" % (name, total))
    if out_f32 is True:
        out_f32 = torch.empty(total, dtype=torch.float32, device=device)
    elif out_f32 is False:
        out_f32 = None
    elif out_f32.dtype != torch.float32 or out_f32.dim() != 1 or not out_f32.is_contiguous() or out_f32.numel() < total:
        raise ValueError("%s: out_f32 must be a contiguous 1-D float32 tensor of out_pcm's size" % name)
    return out_pcm, out_offsets, out_f32


def table_floats(kind, cfg):      # xv_<kind>_table_floats(cfg): the floats of the constant tables of "mfcc", "fbank" or "resample"
    name = "xv_%s_table_floats" % kind
    n = int(getattr(_lib.load(), name)(C.byref(cfg)))
    if n == 0:
        _lib.check(2, name)
    return n


def config_tables(kind, cfg):
    """The constant tables of xv_<kind> for cfg as a host float32 array (xv_<kind>_tables: host arithmetic, no GPU call)."""
    flat = np.empty(table_floats(kind, cfg), np.float32)
    name = "xv_%s_tables" % kind
    _lib.check(getattr(_lib.load(), name)(C.byref(cfg), C.c_void_p(flat.ctypes.data), C.c_size_t(flat.size)), name)
    return flat


def holds_tables(t, floats):      # t is config_tables' array as the kernels read it: `floats` contiguous float32 values
    return t.dtype == torch.float32 and t.is_contiguous() and t.numel() == floats


def pitch4(d):      # d rounded up to 4 floats: the row pitch of a GEMM operand
    return (d + 3) // 4 * 4


def exclusive_offsets(lengths):      # where each of a non-empty list of signals starts when they lie back to back (int64)
    return np.concatenate([[0], np.cumsum(lengths)[:-1]]).astype(np.int64)


def bounds(lengths):      # ... and where each ends: the int64 [b + 1] prefix, item i is bounds[i] .. bounds[i + 1]
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


def greedy_batches(n_items, grow, cost_of, limit, max_items=None, too_big=None):
    """Cuts items 0 .. n_items - 1, in order, into lists that each cost `limit` at the most and hold at most max_items.  The caller keeps
    running totals of a batch as a tuple: grow(i, *totals) -> the totals with item i added (grow(i): of item i alone), cost_of(*totals) ->
    the cost of such a batch.  An item that does not fit alone is refused with too_big(i, its cost), when the batches come to it."""
    batch, totals = [], ()
    for i in range(n_items):
        alone = grow(i)
        if cost_of(*alone) > limit:
            raise ValueError(too_big(i, cost_of(*alone)))
        grown = grow(i, *totals) if batch else alone
        if cost_of(*grown) > limit or len(batch) == max_items:
            yield batch
            batch, grown = [], alone
        batch.append(i)
        totals = grown
    if batch:
        yield batch


def steps(n, step):      # (j0, j1) of 0 .. n in runs of `step`, the last one shorter
    return ((j0, min(j0 + step, n)) for j0 in range(0, n, step))


def cat(parts):      # the results of a loop over steps() as one array or tensor; a single part is passed on as it is
    if len(parts) == 1:
        return parts[0]
    return torch.cat(parts) if parts and isinstance(parts[0], torch.Tensor) else np.concatenate(parts)
