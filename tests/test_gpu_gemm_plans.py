"""Every launch plan of the fp32 GEMMs against the float64 oracle, one row per branch (csrc/xv_gemm_nt.hip xv_nt_plan, csrc/xv_gemm_tn.hip xv_tn_plan).

Each row names the plan it must land on; the test first asserts that plan through the library's own diagnostics (xv_debug_nt_schedule,
xv_debug_tn_plan) and the Python restatement (tests/test_gemm_plans.py) - a row whose shape has drifted off its branch after a plan change
FAILS and says so - and then compares the op-level result with oracle.conv1d_valid_fwd / conv1d_valid_bwd at the GEMM tolerances of
tests/test_gpu_ops.py (5e-6 Frobenius, 2e-5 max).  Every row is launched twice and must reproduce its first result bit for bit (the
hand-over branches - shared SK tiles, shares, split-K, TN splits - sum slabs whose order is fixed).

Coverage (NT kind x launch):         forward + stats      forward, no stats      data gradient (beside the weight gradient)
  DP   one workgroup per tile        K % 16 = 0/4/8/12      K % 16 = 4              K % 16 = 0 (S1 size), 12 (o 1500); N % 4 != 0
  SK   even schedule, shared tiles   yes                    yes, N % 4 != 0         K % 16 = 12 (o 1500), N % 4 != 0
  SK   no shared tiles (tickets null) forced (XV_NT_SCHED=sk, child process): never planned per problem
  SHARES whole tiles + shares        yes, N % 4 != 0        yes, N % 4 != 0         K % 16 = 12 (o 1500), N % 4 != 0
  SPLIT split-K + slab sum           (never with stats)     yes, N % 4 != 0         K % 16 = 12, N % 4 != 0
TN: tn160 (fewer splits than planned, one split), general with and without two-ahead staging, dense one-segment and segmented operands,
segments shorter than a K-step, R % 16 != 0, the few-tile cap, the small-batch wide layer, ZSPLIT and per-row slab sums, l2 = 0 and != 0.
"""
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest
import torch

from oracle import xvector_oracle as O
from tests.test_gemm_plans import NT_NAMES, SK, TN_160, TN_GENERAL, lib_nt, lib_tn, nt_plan, tn_plan, wgrad_reduce_zsplit
from tests.test_gpu_ops import assert_close, dev, host

pytestmark = pytest.mark.gpu

OPS_WS = 256 << 20            # ops.workspace(): the bytes the op-level wrappers plan with


@pytest.fixture(scope="module")
def ops():
    from tf_kaldi_speaker_amd import ops as m
    return m


def c_pad_of(c):
    return (c + 3) // 4 * 4


def nt_problem(op, segs, t_in, c, k, o):
    """(M, N, K, stats, co_running) of xv_affine_forward / xv_affine_dgrad for a layer [segs, t_in, c] -> [segs, t_in - k + 1, o]"""
    if op == "dgrad":
        return segs * t_in, c, k * o, False, True
    return segs * (t_in - k + 1), o, k * c_pad_of(c), op == "fwd_s", False


def assert_nt_plan(name, op, segs, t_in, c, k, o, want, shared=None, forced=0):
    assert forced or "XV_NT_SCHED" not in os.environ, "XV_NT_SCHED forces the NT schedule: the rows need the per-problem choice"
    M, N, K, stats, co = nt_problem(op, segs, t_in, c, k, o)
    got = lib_nt(M, N, K, stats, co)
    pl = nt_plan(M, N, K, stats, co, ws_bytes=OPS_WS, forced=forced)
    msg = "row %s (%s M=%d N=%d K=%d): planned %s, the row is meant for %s - the plan changed; move the row to a shape that still reaches %s" % (
        name, op, M, N, K, NT_NAMES.get(got, got), NT_NAMES[want], NT_NAMES[want])
    assert got == want and pl["kind"] == want, msg
    if want == SK and shared is not None:
        assert pl["shared_tiles"] == shared, "row %s: SK %s shared tiles expected" % (name, "with" if shared else "without")
    return M, N, K


# (name, op, segs, t_in, c, k, o, plan, extra): op fwd_s = forward + BatchNorm statistics, fwd = forward alone, dgrad = data gradient
# (beside the weight gradient); extra: SK rows -> shared tiles expected; forward rows -> ldz (row pitch of z) if not None
NT_ROWS = [
    ("fwd_s-dp-k4-n97", "fwd_s", 1, 16, 20, 1, 97, 0, None),              # K = 20: 20-dim features, one ragged K-step; N % 4 = 1
    ("fwd_s-dp-k4", "fwd_s", 4, 50, 20, 5, 512, 0, None),                # K = 100
    ("fwd_s-dp-k8", "fwd_s", 4, 50, 24, 1, 512, 0, None),                # K = 24
    ("fwd_s-dp-k12-n1499", "fwd_s", 4, 50, 20, 3, 1499, 0, None),        # K = 60, N % 4 = 3
    ("fwd_s-dp-k0-ldz+4", "fwd_s", 4, 50, 30, 5, 1500, 0, 1504),         # K = 160; the engine's 1500 columns on a 1504 pitch
    ("fwd_s-dp-k0-ldz+1", "fwd_s", 4, 50, 30, 5, 1500, 0, 1501),         # odd pitch: the four-byte-store epilogue
    ("fwd_s-sk", "fwd_s", 5, 61, 512, 5, 512, 1, True),
    ("fwd_s-shares-64x200", "fwd_s", 64, 196, 512, 5, 512, 2, None),     # 384 tiles, K = 2560
    ("fwd_s-shares-1tile-per-cu", "fwd_s", 64, 135, 64, 7, 512, 2, None),  # 260 tiles
    ("fwd_s-shares-n97", "fwd_s", 64, 600, 192, 5, 97, 2, None),
    ("fwd_s-shares-n1499-ldz+4", "fwd_s", 1, 5600, 64, 7, 1499, 2, 1503),
    ("fwd-dp-k4", "fwd", 4, 50, 20, 5, 512, 0, None),
    ("fwd-sk", "fwd", 64, 196, 512, 5, 512, 1, True),
    ("fwd-sk-n97", "fwd", 64, 600, 192, 5, 97, 1, True),
    ("fwd-shares", "fwd", 1, 5600, 512, 1, 1500, 2, None),
    ("fwd-shares-n1499", "fwd", 1, 5600, 64, 7, 1499, 2, None),
    ("fwd-split", "fwd", 5, 61, 512, 5, 512, 3, None),
    ("fwd-split-n1499", "fwd", 1, 333, 512, 1, 1499, 3, None),
    ("fwd-split-ldz+4", "fwd", 1, 333, 512, 1, 1500, 3, 1504),
    ("dgrad-dp-o1500-k12", "dgrad", 32, 196, 1500, 1, 1500, 0, None),     # K = 1500: a DP data gradient beside the stream
    ("dgrad-dp-n30", "dgrad", 130, 600, 30, 1, 512, 0, None),
    ("dgrad-sk-o1500-k12", "dgrad", 16, 196, 1500, 1, 1500, 1, True),     # tdnn5 at 16 chunks: the ragged last K-step of the SK kernel
    ("dgrad-sk-n30", "dgrad", 64, 600, 30, 1, 1500, 1, True),
    ("dgrad-sk-n1499", "dgrad", 16, 196, 1499, 1, 1500, 1, True),
    ("dgrad-sk-c192", "dgrad", 130, 135, 192, 5, 512, 1, True),
    ("dgrad-shares-o1500-k12", "dgrad", 32, 200, 1500, 5, 1500, 2, None),  # K = 7500
    ("dgrad-shares-n30", "dgrad", 130, 600, 30, 5, 512, 2, None),
    ("dgrad-split-o1500-k12", "dgrad", 1, 333, 512, 1, 1500, 3, None),
    ("dgrad-split-n1499", "dgrad", 1, 333, 1499, 1, 1500, 3, None),
    ("dgrad-split-n30", "dgrad", 3, 40, 30, 5, 512, 3, None),
]

# the S1 data gradient of tdnn2 (25 088 x 512 x 2 560, one workgroup per tile beside the weight-gradient stream) and the weight gradient
# beside it; its float64 reference is most of this file's time
S1_ROW = ("dgrad-dp-S1", "dgrad", 128, 196, 512, 5, 512, 0, None)


def _layer(seed, segs, t_in, c, k, o):
    rs = np.random.RandomState(seed)
    x = rs.randn(segs, t_in, c).astype(np.float32)
    kern = (rs.randn(k, c, o) / np.sqrt(k * c)).astype(np.float32)
    bias = rs.randn(o).astype(np.float32)
    dz = rs.randn(segs, t_in - k + 1, o).astype(np.float32)
    return rs, x, kern, bias, dz


def _padded_dz(ops, dz, k):
    segs, t_out, o = dz.shape
    pad = k - 1
    dzp = np.zeros((segs, t_out + 2 * pad, o), np.float32)
    dzp[:, pad:pad + t_out] = dz
    return dev(dzp.reshape(-1, o))


def run_nt_row(ops, row, forced=0):
    name, op, segs, t_in, c, k, o, want, extra = row
    assert_nt_plan(name, op, segs, t_in, c, k, o, want, shared=extra if want == SK else None, forced=forced)
    rs, x, kern, bias, dz = _layer(zlib.crc32(name.encode()), segs, t_in, c, k, o)
    x64, k64 = x.astype(np.float64), kern.astype(np.float64)
    if op == "dgrad":
        wf = ops.prep_weight_dgrad(dev(kern))
        d_dzp = _padded_dz(ops, dz, k)
        first = ops.affine_dgrad(d_dzp, segs, t_in - k + 1, o, k, wf, c).clone()
        again = ops.affine_dgrad(d_dzp, segs, t_in - k + 1, o, k, wf, c)
        dx_ref = O.conv1d_valid_bwd(x64, k64, dz.astype(np.float64))[0].reshape(-1, c)
        assert_close(host(first), dx_ref, name="%s: affine_dgrad" % name)
        assert torch.equal(first, again), "%s: the second launch differs from the first" % name
        return
    c_pad = c_pad_of(c)
    xp = ops.pad_channels(dev(x.reshape(-1, c)), c_pad).view(segs, t_in, c_pad)
    wt = ops.prep_weight_fwd(dev(kern), c_pad)
    ldz = extra if want != SK else None
    ref = O.conv1d_valid_fwd(x64, k64, bias.astype(np.float64)).reshape(-1, o)
    stats = op == "fwd_s"
    out = [ops.affine_forward(xp, k, wt, dev(bias), o, with_stats=stats, ldz=ldz) for _ in range(2)]
    if stats:
        (z, part), (z2, part2) = out
        assert torch.equal(part, part2), "%s: the second launch's BatchNorm partials differ from the first" % name
    else:
        z, z2 = out
    assert z.stride(0) == (ldz or o)
    assert_close(host(z), ref, name="%s: affine_forward" % name)
    assert torch.equal(z, z2), "%s: the second launch differs from the first" % name
    if stats:
        rows = ref.shape[0]
        gamma, beta = rs.rand(o).astype(np.float32) + 0.5, rs.randn(o).astype(np.float32)
        mean, invstd, _, _ = ops.bn_finalize(part, rows, dev(gamma), dev(beta), 1e-3, 0.99, True, dev(np.zeros(o)), dev(np.ones(o)))
        assert_close(host(mean), ref.mean(0), 2e-5, 1e-4, "%s: bn mean" % name)
        assert_close(host(invstd), 1 / np.sqrt(ref.var(0) + 1e-3), 2e-5, 1e-4, "%s: bn invstd" % name)


@pytest.mark.parametrize("row", NT_ROWS, ids=[r[0] for r in NT_ROWS])
def test_nt_plan_row(ops, row):
    run_nt_row(ops, row)


def test_nt_row_pitch_leaves_the_padding_columns_alone(ops):
    """ldz > o: the launch writes columns 0 .. o-1 of every row and nothing beyond (the engine keeps other data there)"""
    for o, ldz, want in ((1500, 1504, 0), (1499, 1503, 2), (1500, 1501, 0)):
        segs, t_in, c, k = (4, 50, 30, 5) if want == 0 else (1, 5600, 64, 7)
        assert_nt_plan("ldz %d/%d" % (o, ldz), "fwd_s", segs, t_in, c, k, o, want)
        rs, x, kern, bias, _ = _layer(o + ldz, segs, t_in, c, k, o)
        c_pad = c_pad_of(c)
        xp = ops.pad_channels(dev(x.reshape(-1, c)), c_pad).view(segs, t_in, c_pad)
        wt = ops.prep_weight_fwd(dev(kern), c_pad)
        rows = segs * (t_in - k + 1)
        z = torch.full((rows, ldz), float("nan"), device="cuda")
        part = torch.empty((4, (rows + 127) // 128, o), device="cuda")
        wp, wb = ops._ws(xp)
        ops._lib.call("xv_affine_forward", ops._s(), ops._p(xp), segs, t_in, c_pad, k, ops._p(wt), ops._p(dev(bias)), ops._p(z), o, ldz,
                      ops._p(part), wp, wb)
        zh = host(z)
        assert np.isnan(zh[:, o:]).all(), "ldz %d: columns beyond o were written" % ldz
        ref = O.conv1d_valid_fwd(x.astype(np.float64), kern.astype(np.float64), bias.astype(np.float64)).reshape(-1, o)
        assert_close(zh[:, :o], ref, name="affine_forward ldz %d" % ldz)


def test_nt_sk_without_shared_tiles():
    """The even schedule with every workgroup on whole tiles (tickets = null): the per-problem planner never picks it (a launch without
    shared tiles is never cheaper than one workgroup per tile), so it is forced with XV_NT_SCHED=sk, read once per process - a child."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from tf_kaldi_speaker_amd import ops\n"
            "from tests.test_gpu_gemm_plans import run_nt_row\n"
            "run_nt_row(ops, ('fwd_s-sk-whole-tiles', 'fwd_s', 1, 12288, 512, 1, 1024, 1, False), forced=2)\n"      # 768 tiles x 32 K-steps
            "run_nt_row(ops, ('fwd-sk-two-tiles-each', 'fwd', 1, 24576, 128, 1, 1024, 1, False), forced=2)\n"      # 1 536 tiles: two per workgroup
            "run_nt_row(ops, ('dgrad-sk-whole-tiles', 'dgrad', 1, 12288, 1024, 1, 512, 1, False), forced=2)\n"
            "print('ROWS OK')\n" % root)
    env = dict(os.environ, XV_NT_SCHED="sk")
    r = subprocess.run([sys.executable, "-c", code], cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ROWS OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def test_s1_data_and_weight_gradient(ops):
    name, op, segs, t_in, c, k, o, want, _ = S1_ROW
    assert_nt_plan(name, op, segs, t_in, c, k, o, want)
    M, N, R = k * c, o, segs * (t_in - k + 1)
    assert lib_tn(M, N, R, False) == tn_plan(M, N, R) and lib_tn(M, N, R, False)[0] == TN_GENERAL
    rs, x, kern, _, dz = _layer(2560, segs, t_in, c, k, o)
    dx_ref, dk_ref, _ = O.conv1d_valid_bwd(x.astype(np.float64), kern.astype(np.float64), dz.astype(np.float64))
    d_dzp = _padded_dz(ops, dz, k)
    wf = ops.prep_weight_dgrad(dev(kern))
    dx = ops.affine_dgrad(d_dzp, segs, t_in - k + 1, o, k, wf, c)
    assert_close(host(dx), dx_ref.reshape(-1, c), name="S1 affine_dgrad")
    xp = dev(x)
    dk = ops.affine_wgrad(xp, k, c, d_dzp, t_in - k + 1 + 2 * (k - 1), k - 1, o, dev(kern), 1e-2)
    assert_close(host(dk), dk_ref + 1e-2 * kern.astype(np.float64), name="S1 affine_wgrad")


# ---- TN: weight gradients -------------------------------------------------------------------------------------------------------------
# (name, segs, t_in, c, k, o, (kernel, splits, chunk, ahead), zsplit, l2)
TN_ROWS = [
    ("tn160-fewer-splits-zsplit", 40, 150, 28, 5, 512, (TN_160, 73, 80, 0), True, 1e-2),         # 91 splits planned, 73 cover R
    ("tn160-one-split-r12", 3, 40, 30, 5, 512, (TN_160, 1, 112, 0), False, 0.0),                  # R = 108
    ("general-ahead-dense-cap16", 1, 4096, 512, 1, 512, (TN_GENERAL, 16, 256, 1), False, 0.0),    # 16 tiles: 16 splits, one segment
    ("general-segmented-r13", 5, 61, 512, 5, 512, (TN_GENERAL, 9, 32, 0), False, 1e-2),           # R = 285
    ("general-short-segments", 7, 16, 64, 7, 96, (TN_GENERAL, 2, 48, 0), False, 1e-2),            # 10 frames per segment < a K-step
    ("general-small-batch-wide", 2, 106, 512, 7, 1500, (TN_GENERAL, 3, 80, 0), False, 0.0),       # 336 tiles at R = 200
    ("general-cap-zsplit", 1, 2000, 256, 1, 512, (TN_GENERAL, 32, 64, 0), True, 1e-2),            # 8 tiles: 32 splits
    ("general-dense-r13", 1, 333, 512, 1, 1500, (TN_GENERAL, 7, 48, 0), False, 1e-2),
]


@pytest.mark.parametrize("row", TN_ROWS, ids=[r[0] for r in TN_ROWS])
def test_tn_plan_row(ops, row):
    name, segs, t_in, c, k, o, want, zsplit, l2 = row
    M, N, R = k * c_pad_of(c), o, segs * (t_in - k + 1)
    got = lib_tn(M, N, R, False)
    assert got == want and tn_plan(M, N, R) == want, \
        "row %s (M=%d N=%d R=%d): planned %s, the row is meant for %s - the plan changed; move the row to a shape that still reaches it" % (
            name, M, N, R, got, want)
    assert wgrad_reduce_zsplit(want[1], k, c, o) == zsplit, "row %s: the slab sum is no longer the %s form" % (name, "ZSPLIT" if zsplit else "per-row")
    rs, x, kern, _, dz = _layer(zlib.crc32(name.encode()), segs, t_in, c, k, o)
    _, dk_ref, _ = O.conv1d_valid_bwd(x.astype(np.float64), kern.astype(np.float64), dz.astype(np.float64))
    c_pad = c_pad_of(c)
    xp = ops.pad_channels(dev(x.reshape(-1, c)), c_pad).view(segs, t_in, c_pad)
    d_dzp = _padded_dz(ops, dz, k)
    t_out = t_in - k + 1
    args = (xp, k, c, d_dzp, t_out + 2 * (k - 1), k - 1, o, dev(kern), l2)
    first = ops.affine_wgrad(*args).clone()
    again = ops.affine_wgrad(*args)
    assert_close(host(first), dk_ref + l2 * kern.astype(np.float64), name="%s: affine_wgrad" % name)
    assert torch.equal(first, again), "%s: the second launch differs from the first" % name
