"""CPU tests of the host side of the diarization ops (the clusterers, the cluster sums, VBx, the per-recording PCA): what each op hands to
its C entry point, every refusal that comes before a launch, and the caps.  Tensors live on the CPU (or on the meta device, where only
a size matters) and nothing is launched.

The launch trace and the refusals ask the same of any commit: they find the ops' module through ops.vbx.__module__ and pass on the
commit before the ops were split out of pipeline_ops.py, where tests/golden/diar_launches.json was recorded by running this file as a
script.  The caps test reads the constants of _lib.py."""
import contextlib
import ctypes as C
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, ROOT)

from tf_kaldi_speaker_amd import _lib, ops      # noqa: E402

M = sys.modules[ops.vbx.__module__]      # the module of the diarization ops
GOLDEN = os.path.join(ROOT, "tests", "golden", "diar_launches.json")
SUMS_STATUS = 18      # xv_ahc_cluster_sums: the position of `status`, which the op reads back before it returns


# ---- the recorder ---------------------------------------------------------------------------------------------------------------
class _Ptr(object):
    """What the substituted _p hands on: the tensor itself (None: a null pointer)."""

    def __init__(self, t):
        self.t = t


def _tensor(t):
    out = {"dtype": str(t.dtype).replace("torch.", ""), "shape": list(t.shape)}
    if t.dtype.is_floating_point:
        out["nan"] = bool(t.numel() > 0 and torch.isnan(t).all())      # (an uninitialised tensor is zero here: _traced)
    else:
        out["values"] = t.reshape(-1).tolist()
    return out


def _argument(a):
    if isinstance(a, _Ptr):
        return None if a.t is None else _tensor(a.t)
    if isinstance(a, (C.c_float, C.c_double)):
        return [type(a).__name__, float(a.value).hex()]
    if isinstance(a, C._SimpleCData):
        return [type(a).__name__, a.value]
    if type(a) in (int, str):
        return [type(a).__name__, a]
    return ["unexpected " + type(a).__name__, repr(a)]      # (a NumPy scalar, say: ctypes would not take it)


@contextlib.contextmanager
def _traced(sums_status=None):
    """The ops' module with _lib.call as a recorder, _s as a constant and _p as _Ptr; torch.empty gives zeros, so that the fill of what
    an op allocates (NaN / -1 / none) reads the same in every run.  -> the list of launches; each keeps its tensors under "held"."""
    launches, lib = [], M._lib

    def call(name, *args):
        launches.append({"entry": name, "args": [_argument(a) for a in args], "held": args})
        if name == "xv_ahc_cluster_sums":
            args[SUMS_STATUS].t.zero_()
            if sums_status is not None:
                args[SUMS_STATUS].t.copy_(torch.tensor(sums_status, dtype=torch.int32))

    saved = lib.call, M._s, M._p, torch.empty, torch.empty_like
    lib.call, M._s, M._p = call, (lambda: "stream"), _Ptr
    torch.empty = lambda *a, **kw: saved[3](*a, **kw).zero_()
    torch.empty_like = lambda *a, **kw: saved[4](*a, **kw).zero_()
    try:
        yield launches
    finally:
        lib.call, M._s, M._p, torch.empty, torch.empty_like = saved


def _record(op, *args, **kw):
    """One op call under the recorder -> {"launches": ..., "returns": the dtype and shape of each tensor that comes back, and the argument
    of the last launch that it is}."""
    with _traced() as launches:
        got = op(*args, **kw)
    last = [a.t.data_ptr() if isinstance(a, _Ptr) and a.t is not None and a.t.numel() else None for a in launches[-1]["held"]]

    def returned(t):
        return {"dtype": str(t.dtype).replace("torch.", ""), "shape": list(t.shape), "arg": last.index(t.data_ptr()) if t.data_ptr() in last else None}
    returns = {k: returned(v) for k, v in got.items()} if isinstance(got, dict) else [returned(v) for v in got]
    return {"launches": [{"entry": l["entry"], "args": l["args"]} for l in launches], "returns": returns}


# ---- the inputs: the smallest that reach every branch ------------------------------------------------------------------------------
def _f32(n, seed):
    return torch.from_numpy(np.random.RandomState(seed).randn(n).astype(np.float32))


def _f64(shape, seed):
    return torch.from_numpy(np.random.RandomState(seed).randn(*shape))


N, OFF, LD = [1, 2, 5], [2, 8, 20], [4, 4, 8]      # three matrices with gaps between them, inside 64 floats on either pitch
SUMS_N, SUMS_OFF, SUMS_LD, SUMS_LABELS = [3, 5], [1, 20], [4, 8], [0, 1, 0, 0, 1, 1, 2, 0]
T, S, D, X_OFF, X_LD = [1, 4], [1, 2], 3, [1, 8], [4, 7]      # two recordings of rows inside 40 floats on either pitch


def _vbx_inputs(t=T, s=S, d=D):
    ts = int(sum(a * b for a, b in zip(t, s)))
    return dict(x=_f32(40, 5), x_offsets=X_OFF, t=t, d=d, phi=_f32(d, 6).abs(), gamma=_f32(ts, 7).abs(), pi=_f32(int(sum(s)), 8).abs(), s=s)


def _pca_inputs(d=D):
    return dict(x=_f32(40, 5), x_offsets=X_OFF, n=T, d=d, w=_f64((d, d), 9), b=_f64((d, d), 10), mu=_f64((d,), 11), target=0.9)


def trace_all():
    out, scores = {}, _f32(64, 3)
    for tag, ld in (("ld_none", None), ("ld_given", LD)):
        out["ahc_cluster/%s/no_targets" % tag] = _record(ops.ahc_cluster, scores, OFF, N, ld, threshold=0.25)
        out["ahc_cluster/%s/targets" % tag] = _record(ops.ahc_cluster, scores, OFF, N, ld, threshold=0.25, targets=[0, 1, 3])
        out["ahc_cluster_from/%s/floors" % tag] = _record(ops.ahc_cluster_from, scores, OFF, N, ld, floors=[1, 2, 2])
        members, starts, c = ops.ahc_member_lists(SUMS_LABELS, SUMS_N)
        out["ahc_cluster_sums/%s" % tag] = _record(ops.ahc_cluster_sums, scores, SUMS_OFF, SUMS_N, SUMS_LD if ld else None, members, starts, c)
        out["vbx/%s" % tag] = _record(ops.vbx, ld=X_LD if ld else None, max_iters=7, **_vbx_inputs())
        out["backend_pca_plda/%s" % tag] = _record(ops.backend_pca_plda, ld=X_LD if ld else None, **_pca_inputs())
    out["ahc_cluster_from/ld_none/no_floors"] = _record(ops.ahc_cluster_from, scores, OFF, N, threshold=0.5)
    out["ahc_cluster_from/seeded"] = _record(ops.ahc_cluster_from, None, None, [2, 3], floors=[1, 2], seed=_f32(13, 4), sizes=[1, 2, 1, 1, 3])
    out["ahc_member_lists"] = [a.tolist() + [str(a.dtype)] for a in ops.ahc_member_lists(SUMS_LABELS, SUMS_N)]
    return json.loads(json.dumps(out))


def test_the_launches_are_the_recorded_ones():
    """Entry point, order, every scalar, the contents of every uploaded index array and the dtype, shape and fill of every output, for
    each op and each branch of its host code, against the record of the ops as they stood in pipeline_ops.py."""
    with open(GOLDEN, "r") as f:
        want = json.load(f)
    got = trace_all()
    assert sorted(got) == sorted(want)
    for case in want:
        assert got[case] == want[case], case
    assert torch.empty(3).dtype == torch.float32 and M._lib.call is _lib.call and not isinstance(M._p(None), _Ptr)      # the recorder is gone


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def _meta(floats):      # a buffer of which the checks read the size only
    return torch.empty(int(floats), dtype=torch.float32, device="meta")


def _refused(cases):
    for exc, text, call in cases:
        with pytest.raises(exc, match="^%s$" % re.escape(text)):
            call()


def _buffer_refusals(name, what, call):      # call(buffer)
    text = "%s: %s must be a non-empty contiguous 1-D float32 tensor" % (name, what)
    return [(ValueError, text, lambda bad=bad: call(bad)) for bad in (torch.zeros(64, dtype=torch.float64), torch.zeros(8, 8), torch.zeros(0), torch.zeros(128)[::2])]


def _matrix_refusals(name, cap, call):
    """The refusals of b square matrices in one buffer: call(scores, mat_offsets, n, ld) is the op with valid arguments otherwise."""
    scores = _f32(64, 3)
    return _buffer_refusals(name, "scores", lambda bad: call(bad, OFF, N, LD)) + [
        (ValueError, "%s: n must be a non-empty 1-D integer array" % name, lambda: call(scores, [], [], None)),
        (ValueError, "%s: n must be a non-empty 1-D integer array" % name, lambda: call(scores, OFF, [1.0, 2.0, 5.0], LD)),
        (ValueError, "%s: recording 1 has no row (n = 0)" % name, lambda: call(scores, OFF, [1, 0, 5], None)),
        (ValueError, "%s: recording 0 has %d rows, the cap is %d" % (name, cap + 1, cap), lambda: call(_meta((cap + 1) ** 2), [0], [cap + 1], None)),
        (ValueError, "%s: ld must be a 1-D integer array of 3" % name, lambda: call(scores, OFF, N, [4, 4])),
        (ValueError, "%s: recording 2: the pitch 4 is below its 5 rows" % name, lambda: call(scores, OFF, N, [4, 4, 4])),
        (ValueError, "%s: mat_offsets must be a 1-D integer array of 3" % name, lambda: call(scores, [2, 8], N, LD)),
        (IndexError, "%s: a matrix lies outside the 64 floats of scores" % name, lambda: call(scores, [2, 8, 28], N, LD)),
        (IndexError, "%s: a matrix lies outside the 64 floats of scores" % name, lambda: call(scores, [-1, 8, 20], N, LD)),
    ]


def _rows_refusals(name, letter, cap, call):
    """The refusals of b recordings of rows [n_i, ld_i] of d = 3 floats in one buffer: call(x, x_offsets, n, ld)."""
    x = _f32(40, 5)
    return _buffer_refusals(name, "x", lambda bad: call(bad, X_OFF, T, X_LD)) + [
        (ValueError, "%s: %s must be a non-empty 1-D integer array" % (name, letter), lambda: call(x, [], [], None)),
        (ValueError, "%s: recording 1 has no row (%s = 0)" % (name, letter), lambda: call(x, X_OFF, [1, 0], None)),
        (ValueError, "%s: recording 0 has %d rows, the cap is %d" % (name, cap + 1, cap), lambda: call(_meta(3 * (cap + 1)), [0], [cap + 1], None)),
        (ValueError, "%s: ld must be a 1-D integer array of 2" % name, lambda: call(x, X_OFF, T, [4])),
        (ValueError, "%s: recording 1: the pitch 2 is below the 3 dimensions" % name, lambda: call(x, X_OFF, T, [4, 2])),
        (ValueError, "%s: x_offsets must be a 1-D integer array of 2" % name, lambda: call(x, [1], T, X_LD)),
        (IndexError, "%s: a recording's rows lie outside the 40 floats of x" % name, lambda: call(x, [1, 17], T, X_LD)),
        (IndexError, "%s: a recording's rows lie outside the 40 floats of x" % name, lambda: call(x, [-1, 8], T, X_LD)),
    ]


def test_ahc_cluster_refuses_as_before():
    scores = _f32(64, 3)
    _refused(_matrix_refusals("ahc_cluster", 2048, lambda s, off, n, ld: ops.ahc_cluster(s, off, n, ld)) + [
        (ValueError, "ahc_cluster: targets must be a 1-D integer array of 3", lambda: ops.ahc_cluster(scores, OFF, N, LD, targets=[0, 1])),
        (ValueError, "ahc_cluster: recording 1: target 3 outside 0 .. 2", lambda: ops.ahc_cluster(scores, OFF, N, LD, targets=[0, 3, 5])),
        (ValueError, "ahc_cluster: recording 2: target -1 outside 0 .. 5", lambda: ops.ahc_cluster(scores, OFF, N, LD, targets=[0, 0, -1])),
    ])


def test_ahc_cluster_from_refuses_as_before():
    name, scores, seed, sizes = "ahc_cluster_from", _f32(64, 3), _f32(13, 4), [1, 2, 1, 1, 3]
    seeded = lambda n=(2, 3), seed=seed, sizes=sizes, **kw: ops.ahc_cluster_from(None, None, list(n), seed=seed, sizes=sizes, **kw)
    _refused(_matrix_refusals(name, 2048, lambda s, off, n, ld: ops.ahc_cluster_from(s, off, n, ld)) + [
        (ValueError, name + ": sizes belong to a seeded start (seed is None)", lambda: ops.ahc_cluster_from(scores, OFF, N, LD, sizes=[1] * 8)),
        (ValueError, name + ": floors must be a 1-D integer array of 3", lambda: ops.ahc_cluster_from(scores, OFF, N, LD, floors=[1, 1])),
        (ValueError, name + ": recording 1: floor 3 outside 1 .. 2", lambda: ops.ahc_cluster_from(scores, OFF, N, LD, floors=[1, 3, 2])),
        (ValueError, name + ": recording 0: floor 0 outside 1 .. 1", lambda: ops.ahc_cluster_from(scores, OFF, N, LD, floors=[0, 1, 2])),
        (ValueError, name + ": the threshold is NaN", lambda: ops.ahc_cluster_from(scores, OFF, N, LD, threshold=float("nan"))),
        (ValueError, name + ": the threshold is NaN", lambda: seeded(threshold=float("nan"))),
        (ValueError, name + ": a seeded start reads no scores (scores, mat_offsets and ld must be None)",
         lambda: ops.ahc_cluster_from(scores, None, [2, 3], seed=seed, sizes=sizes)),
        (ValueError, name + ": a seeded start reads no scores (scores, mat_offsets and ld must be None)",
         lambda: ops.ahc_cluster_from(None, [0, 4], [2, 3], seed=seed, sizes=sizes)),
        (ValueError, name + ": a seeded start reads no scores (scores, mat_offsets and ld must be None)",
         lambda: ops.ahc_cluster_from(None, None, [2, 3], [2, 3], seed=seed, sizes=sizes)),
        (ValueError, name + ": n must be a non-empty 1-D integer array", lambda: seeded(n=(), sizes=[])),
        (ValueError, name + ": recording 1 has 0 clusters, 1 .. 2048 are taken", lambda: seeded(n=(2, 0), sizes=[1, 2])),
        (ValueError, name + ": recording 0 has 2049 clusters, 1 .. 2048 are taken", lambda: seeded(n=(2049,), seed=_meta(2049 ** 2), sizes=[1] * 2049)),
        (ValueError, name + ": seed must be a contiguous 1-D float32 tensor of at least 13 floats", lambda: seeded(seed=seed[:12])),
        (ValueError, name + ": seed must be a contiguous 1-D float32 tensor of at least 13 floats", lambda: seeded(seed=seed.double())),
        (ValueError, name + ": seed must be a contiguous 1-D float32 tensor of at least 13 floats", lambda: seeded(seed=torch.zeros(13, 2)[:, 0])),
        (ValueError, name + ": sizes must be a 1-D integer array of 5", lambda: seeded(sizes=None)),
        (ValueError, name + ": sizes must be a 1-D integer array of 5", lambda: seeded(sizes=[1, 2, 1, 1])),
        (ValueError, name + ": recording 1: the sizes must be positive and add up to at most 32768", lambda: seeded(sizes=[1, 2, 1, 0, 3])),
        (ValueError, name + ": recording 0: the sizes must be positive and add up to at most 32768", lambda: seeded(sizes=[32767, 2, 1, 1, 3])),
        (ValueError, name + ": floors must be a 1-D integer array of 2", lambda: seeded(floors=[1])),
        (ValueError, name + ": recording 1: floor 4 outside 1 .. 3", lambda: seeded(floors=[1, 4])),
    ])


def test_ahc_member_lists_refuses_as_before():
    _refused([
        (ValueError, "ahc_member_lists: n must be a non-empty 1-D integer array", lambda: ops.ahc_member_lists([], [])),
        (ValueError, "ahc_member_lists: labels must be a 1-D integer array of 8", lambda: ops.ahc_member_lists(SUMS_LABELS[:7], SUMS_N)),
        (ValueError, "ahc_member_lists: a recording's labels must be 0, 1, ... in the order of the clusters' smallest members",
         lambda: ops.ahc_member_lists([1, 0, 0, 0, 1, 1, 2, 0], SUMS_N)),
        (ValueError, "ahc_member_lists: a recording's labels must be 0, 1, ... in the order of the clusters' smallest members",
         lambda: ops.ahc_member_lists([0, 2, 2, 0, 1, 1, 2, 0], SUMS_N)),
    ])


def _single_cluster_lists(n):      # every recording one cluster of all its rows: valid lists for any n >= 1
    n = [int(r) for r in n]
    members = np.concatenate([np.arange(r) for r in n] or [np.zeros(0, np.int64)])
    return members, np.asarray([v for r in n for v in (0, r)], np.int64), [1] * len(n)


def test_ahc_cluster_sums_refuses_as_before():
    name, scores = "ahc_cluster_sums", _f32(64, 3)
    members, starts, c = ops.ahc_member_lists(SUMS_LABELS, SUMS_N)
    sums = lambda members=members, starts=starts, c=c: ops.ahc_cluster_sums(scores, SUMS_OFF, SUMS_N, SUMS_LD, members, starts, c)
    # (where n itself is the fault, no member list fits it: the lists are checked behind the matrices)
    _refused(_matrix_refusals(name, 32768, lambda s, off, n, ld: ops.ahc_cluster_sums(s, off, n, ld, *_single_cluster_lists(np.maximum(np.asarray(n, np.int64), 0)))) + [
        (ValueError, name + ": c must be a 1-D integer array of 2", lambda: sums(c=[2])),
        (ValueError, name + ": recording 0 has 0 clusters, 1 .. 3 are taken", lambda: sums(c=[0, 3])),
        (ValueError, name + ": recording 0 has 4 clusters, 1 .. 3 are taken", lambda: sums(c=[4, 3])),
        (ValueError, name + ": recording 0 has 2049 clusters, 1 .. 2048 are taken",
         lambda: ops.ahc_cluster_sums(_meta(2049 ** 2), [0], [2049], None, np.arange(2049), np.arange(2050), [2049])),
        (ValueError, name + ": members must be a 1-D integer array of 8", lambda: sums(members=members[:7])),
        (ValueError, name + ": starts must be a 1-D integer array of 7", lambda: sums(starts=starts[:6])),
        (ValueError, name + ": recording 0: starts must ascend from 0 to its 3 rows", lambda: sums(starts=[1, 2, 3, 0, 2, 4, 5])),
        (ValueError, name + ": recording 1: starts must ascend from 0 to its 5 rows", lambda: sums(starts=[0, 2, 3, 0, 2, 2, 5])),
        (ValueError, name + ": recording 1: starts must ascend from 0 to its 5 rows", lambda: sums(starts=[0, 2, 3, 0, 2, 4, 4])),
        (ValueError, name + ": recording 0: members must hold every row once, clusters ascending by their smallest member, a cluster's members ascending",
         lambda: sums(members=[0, 2, 2, 0, 4, 1, 2, 3])),
        (ValueError, name + ": recording 0: members must hold every row once, clusters ascending by their smallest member, a cluster's members ascending",
         lambda: sums(members=[2, 0, 1, 0, 4, 1, 2, 3])),
        (ValueError, name + ": recording 1: members must hold every row once, clusters ascending by their smallest member, a cluster's members ascending",
         lambda: sums(members=[0, 2, 1, 1, 2, 0, 4, 3])),
    ])
    assert members.tolist() == [0, 2, 1, 0, 4, 1, 2, 3] and starts.tolist() == [0, 2, 3, 0, 2, 4, 5] and c.tolist() == [2, 3]
    with _traced(sums_status=[0, -1]):      # what the op says of a recording the kernel skipped
        with pytest.raises(RuntimeError, match="^ahc_cluster_sums: xv_ahc_cluster_sums skipped recording 1$"):
            sums()


def test_ahc_cluster_two_pass_refuses_as_before():
    name, scores = "ahc_cluster_two_pass", _f32(64, 3)
    two = lambda **kw: ops.ahc_cluster_two_pass(scores, OFF, N, LD, **kw)
    _refused(_matrix_refusals(name, 32768, lambda s, off, n, ld: ops.ahc_cluster_two_pass(s, off, n, ld)) + [
        (ValueError, name + ": first_pass_max_points must lie in 2 .. 2048 (got 1)", lambda: two(first_pass_max_points=1)),
        (ValueError, name + ": first_pass_max_points must lie in 2 .. 2048 (got 2049)", lambda: two(first_pass_max_points=2049)),
        (ValueError, name + ": targets must be a 1-D integer array of 3", lambda: two(targets=[1, 1])),
        (ValueError, name + ": recording 1: target 3 outside 1 .. 2 (None: the threshold, for every recording)", lambda: two(targets=[1, 3, 1])),
        (ValueError, name + ": recording 0: target 0 outside 1 .. 1 (None: the threshold, for every recording)", lambda: two(targets=[0, 1, 1])),
    ])


def test_vbx_refuses_as_before():
    vbx = lambda ld=None, **kw: ops.vbx(ld=ld, **dict(_vbx_inputs(), **kw))
    wide = lambda d: ops.vbx(_f32(5 * d, 5), [0, d], T, d, _f32(d, 6).abs(), _f32(9, 7).abs(), _f32(3, 8).abs(), S)

    def rows(x, x_offsets, t, ld):      # (one speaker each: gamma and pi fit whatever t holds)
        return ops.vbx(x, x_offsets, t, D, _f32(D, 6).abs(), _f32(max(sum(t), 1), 7).abs(), _f32(max(len(t), 1), 8).abs(), [1] * len(t), ld=ld)
    _refused(_rows_refusals("vbx", "t", 2048, rows) + [
        (ValueError, "vbx: d must lie in 1 .. 256 (got 0)", lambda: vbx(d=0)),
        (ValueError, "vbx: d must lie in 1 .. 256 (got 257)", lambda: wide(257)),
        (ValueError, "vbx: max_iters must lie in 1 .. 64 (got 0)", lambda: vbx(max_iters=0)),
        (ValueError, "vbx: max_iters must lie in 1 .. 64 (got 65)", lambda: vbx(max_iters=65)),
        (ValueError, "vbx: loop_prob must lie strictly between 0 and 1 as a float32 (got 0.0)", lambda: vbx(loop_prob=0.0)),
        (ValueError, "vbx: loop_prob must lie strictly between 0 and 1 as a float32 (got 1.0)", lambda: vbx(loop_prob=1.0)),
        (ValueError, "vbx: loop_prob must lie strictly between 0 and 1 as a float32 (got 0.999999999)", lambda: vbx(loop_prob=0.999999999)),
        (ValueError, "vbx: fa and fb must be positive (got 0.0, 17.0)", lambda: vbx(fa=0.0)),
        (ValueError, "vbx: fa and fb must be positive (got 0.3, -1.0)", lambda: vbx(fb=-1.0)),
        (ValueError, "vbx: fa and fb must be positive (got 0.3, inf)", lambda: vbx(fb=float("inf"))),
        (ValueError, "vbx: epsilon is not a number", lambda: vbx(epsilon=float("nan"))),
        (ValueError, "vbx: s must be a 1-D integer array of 2", lambda: vbx(s=[1])),
        (ValueError, "vbx: recording 1 has no speaker (s = 0)", lambda: vbx(s=[1, 0], gamma=_f32(1, 7), pi=_f32(1, 8))),
        (ValueError, "vbx: recording 1 has 33 speakers, the cap is 32", lambda: vbx(s=[1, 33], gamma=_f32(1 + 4 * 33, 7), pi=_f32(34, 8))),
        (ValueError, "vbx: phi must be 3 contiguous float32 values", lambda: vbx(phi=_f32(4, 6))),
        (ValueError, "vbx: phi must be 3 contiguous float32 values", lambda: vbx(phi=_f32(3, 6).double())),
        (ValueError, "vbx: gamma (sum of t * s) must be 9 contiguous float32 values", lambda: vbx(gamma=_f32(8, 7))),
        (ValueError, "vbx: pi (sum of s) must be 3 contiguous float32 values", lambda: vbx(pi=_f32(4, 8))),
    ])


def test_backend_pca_plda_refuses_as_before():
    name = "backend_pca_plda"
    pca = lambda ld=None, **kw: ops.backend_pca_plda(ld=ld, **dict(_pca_inputs(), **kw))
    wide = lambda d: ops.backend_pca_plda(_f32(5 * d, 5), [0, d], T, d, _f64((d, d), 9), _f64((d, d), 10), _f64((d,), 11), 0.9)
    _refused(_rows_refusals(name, "n", 2048, lambda x, x_offsets, n, ld: pca(ld, x=x, x_offsets=x_offsets, n=n)) + [
        (ValueError, name + ": d must lie in 1 .. 256 (got 0)", lambda: pca(d=0)),
        (ValueError, name + ": d must lie in 1 .. 256 (got 257)", lambda: wide(257)),
        (ValueError, name + ": target must lie in (0, 1] (got 0.0)", lambda: pca(target=0.0)),
        (ValueError, name + ": target must lie in (0, 1] (got 1.5)", lambda: pca(target=1.5)),
        (ValueError, name + ": target must lie in (0, 1] (got nan)", lambda: pca(target=float("nan"))),
        (ValueError, name + ": w must be a contiguous float64 [3, 3] tensor on the rows' device", lambda: pca(w=_f64((3, 3), 9).float())),
        (ValueError, name + ": b must be a contiguous float64 [3, 3] tensor on the rows' device", lambda: pca(b=_f64((3, 2), 10))),
        (ValueError, name + ": b must be a contiguous float64 [3, 3] tensor on the rows' device", lambda: pca(b=_f64((3, 3), 10).t())),
        (ValueError, name + ": mu must be a contiguous float64 [3] tensor on the rows' device", lambda: pca(mu=_f64((4,), 11))),
        (ValueError, name + ": w must be a contiguous float64 [3, 3] tensor on the rows' device", lambda: pca(w=_f64((3, 3), 9).to("meta"))),
    ])


def test_score_normalize_refuses_its_scores_as_before():
    stats = torch.ones(2, 2)
    _refused(_buffer_refusals("score_normalize", "scores", lambda bad: ops.score_normalize(bad, [0], [0], stats, stats)))


# ---- the caps ---------------------------------------------------------------------------------------------------------------------
def test_the_caps_are_those_the_entry_points_name():
    """Each cap of _lib.py is the number its C entry point names when it refuses cap + 1.  Every call below also hands over a null buffer,
    which the entry points look at behind their caps: none of them can reach a launch, whatever the constants say."""
    lib, p = _lib.load(), C.c_void_p(4096)

    def says(rc):
        assert rc != 0
        return lib.xv_last_error().decode()

    def ahc(max_n):
        return says(lib.xv_ahc_cluster(None, None, 1, p, p, p, p, 1, max_n, max_n, max_n * max_n, 0.0, p, p, p, p, None, 0))

    def ahc_from(max_n):
        return says(lib.xv_ahc_cluster_from(None, p, 1, p, None, p, p, None, 0, 1, max_n, max_n, max_n * max_n, 0.0, p, p, p, p, None, 0))

    def sums(max_n, max_c):
        return says(lib.xv_ahc_cluster_sums(None, None, 1, p, p, p, p, p, p, 1, max_n, max_c, max_n, max_c, max_c * max_c, max_n * max_c, p, p, p, None, 0))

    def vbx(max_t=4, max_s=2, d=3, max_iters=5):
        return says(lib.xv_vbx(None, None, 1, p, p, p, p, 1, d, max_t, max_s, max_t, max_t * max_s, max_s, p, p, p, 0.5, 0.3, 17.0, max_iters, 1e-4,
                               p, p, p, p, p, None, 0))

    def pca(d=3, max_n=4):
        return says(lib.xv_backend_pca_plda(None, None, 1, p, p, p, 1, d, max_n, 0.9, p, p, p, p, p, p, p, p, p, p, p, p, p, None, 0))

    rows = "%s: a recording of %d rows exceeds the cap of %d"
    cap = _lib.AHC_MAX_N
    assert cap == ops.AHC_MAX_N and rows % ("ahc_cluster", cap + 1, cap) == ahc(cap + 1) and rows % ("ahc_cluster_from", cap + 1, cap) == ahc_from(cap + 1)
    assert sums(cap + 1, cap + 1) == "ahc_cluster_sums: %d clusters exceed the cap of %d (or the %d rows)" % (cap + 1, cap, cap + 1)
    cap = _lib.AHC_MAX_POINTS
    assert cap == ops.AHC_MAX_POINTS and rows % ("ahc_cluster_sums", cap + 1, cap) == sums(cap + 1, 1)
    cap = _lib.VBX_MAX_ROWS
    assert rows % ("vbx", cap + 1, cap) == vbx(max_t=cap + 1)
    cap = _lib.VBX_MAX_SPEAKERS
    assert cap == ops.VBX_MAX_SPEAKERS and vbx(max_s=cap + 1) == "vbx: %d speakers exceed the cap of %d" % (cap + 1, cap)
    cap = _lib.VBX_MAX_DIM
    assert cap == ops.VBX_MAX_DIM and vbx(d=cap + 1) == "vbx: d must lie in 1 .. %d (got %d)" % (cap, cap + 1)
    cap = _lib.VBX_MAX_ITERS
    assert cap == ops.VBX_MAX_ITERS and vbx(max_iters=cap + 1) == "vbx: max_iters must lie in 1 .. %d (got %d)" % (cap, cap + 1)
    cap = _lib.PCA_MAX_ROWS
    assert rows % ("backend_pca_plda", cap + 1, cap) == pca(max_n=cap + 1)
    cap = _lib.PCA_MAX_DIM
    assert cap == ops.PCA_MAX_DIM and pca(d=cap + 1) == "backend_pca_plda: d must lie in 1 .. %d (got %d)" % (cap, cap + 1)
    # with the caps respected, what refuses these calls is the null buffer
    for text in (ahc(_lib.AHC_MAX_N), ahc_from(_lib.AHC_MAX_N), sums(_lib.AHC_MAX_POINTS, _lib.AHC_MAX_N),
                 vbx(_lib.VBX_MAX_ROWS, _lib.VBX_MAX_SPEAKERS, _lib.VBX_MAX_DIM, _lib.VBX_MAX_ITERS), pca(_lib.PCA_MAX_DIM, _lib.PCA_MAX_ROWS)):
        assert text.endswith(": bad arguments"), text


if __name__ == "__main__":      # records the launches of the checked-out commit
    cases = trace_all()
    with open(GOLDEN, "w") as f:
        f.write("{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(cases[k], sort_keys=True)) for k in sorted(cases)) + "\n}\n")
    print("wrote %d cases to %s" % (len(cases), GOLDEN))
