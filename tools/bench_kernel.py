#!/usr/bin/env python3
"""Kernel micro-benchmarks of libxvector_hip.so at the S1 tensor sizes - diagnostics, not tests, not the product path.  One file, one
sub-command per question (they used to be eight scripts):

  python tools/bench_kernel.py gemm [frames=200]                fp32-input MFMA GEMMs per layer: forward / data gradient / weight gradient (incl. slab sum)
  python tools/bench_kernel.py gemm16 [frames=200] [tdnn2,tdnn5] the same for the split-precision (f16x3) kernels
  python tools/bench_kernel.py elementwise [frames=200]         every HBM-bound kernel of the step alone - run under `rocprofv3 --kernel-trace` and feed the
                                                                trace to tools/elementwise_summary.py (prices them against 8 TB/s; north_star asks >= 70 %)
  python tools/bench_kernel.py width                            the row-structured HBM-bound kernels against the channel count (512 ... 3 000)
  python tools/bench_kernel.py pitch                            ... against the row pitch of a 1 500-channel tensor
  python tools/bench_kernel.py pool [frames=186] [channels=1500] statistics pooling (+ BatchNorm) and its backward, warm (Infinity Cache) and cold
  python tools/bench_kernel.py vlad [frames=186] [centers=8] [ghosts=2] GhostVLAD pooling (xv_vlad.hip) at 128 chunks x frames x 1500: the pooling forward and backward
                                                                passes alternated with stat_pool_forward on the same tensor - medians, bytes, ratios
  python tools/bench_kernel.py triplet                          the pairwise loss heads (xv_triplet.hip): forward and backward of every kind at 64 speakers x
                                                                10 segments x 512 and at 128 x 512, the e2e validation loss; warm and cold, alternated rounds
  python tools/bench_kernel.py ge2e                             the GE2E training loss (xv_triplet.hip): forward and backward of both types at 64 x 10 and
                                                                32 x 4 rows x 512, beside the angular head on the same rows; warm and cold
  python tools/bench_kernel.py ge2e steps <parent tree> [rounds]   the S1-shaped step with the GE2E head against the angular-triplet step of a checkout
                                                                of the parent commit, alternated fresh processes
  python tools/bench_kernel.py triplet steps <parent tree> [rounds] the S1-shaped training step with a pairwise head against the AM-Softmax step of a checkout
                                                                of the parent commit and of this tree, fresh processes, alternated
  python tools/bench_kernel.py segment                          the segment-level GEMMs: one-launch form (xv_skinny.hip) against GEMM + slab-sum launches
  python tools/bench_kernel.py staged                           plain step vs the staged (multi-GPU) backward, without / with a one-rank RCCL all-reduce
  python tools/bench_kernel.py score [small|large]              the scoring stage (xv_score.hip) on synthetic unit vectors, d = 512: VoxCeleb1-O-sized and E-sized
  python tools/bench_kernel.py backend [small|large]            the LDA / PLDA back end's device ops (xv_backend.hip) on synthetic vectors, d = 512, LDA to 200
  python tools/bench_kernel.py plda_cohort [small|large]        the cohort statistics of PLDA scores (xv_backend_cohort.hip): d = 200, 4 k rows, cohorts of 4 k / 40 k
  python tools/bench_kernel.py dense [n ...]                     the all-pairs score matrix of one recording (xv_score_dense, xv_backend_plda_dense) at d = 200,
                                                                n = 200 / 800 / 2000 windows, into a view of a packed buffer
  python tools/bench_kernel.py ahc [recordings=64] [n ...]      agglomerative clustering (xv_ahc.hip): one call over 64 recordings of n = 200 / 800 / 2000
                                                                windows, medians over alternated rounds, beside scipy's average linkage on 16 CPUs
  python tools/bench_kernel.py ahc2 [n ...]                     two-pass clustering of one long recording (xv_ahc_cluster_from, xv_ahc_cluster_sums): n = 4096 / 8192
                                                                windows, the stages apart, the single pass at 2048 windows for scale
  python tools/bench_kernel.py diar_tune [recordings=64] [n=600] threshold tuning (xv_ahc_cut, xv_diar_confusion): Diarizer.sweep + DerSweep over 13 thresholds against 13 x
                                                                (Diarizer.cluster + rttm_turns + der()), alternated rounds, the sweep's parts and the two ops alone
  python tools/bench_kernel.py vbx [recordings=64] [T,S ...]     VB-HMM clustering (xv_vbx.hip): one call over 64 recordings at (T, D, S) = (200, 128, 6), (800, 128, 10)
                                                                and (2000, 128, 16), 20 iterations, medians over alternated rounds, beside the float64 NumPy
                                                                restatement of one recording on the CPU
  python tools/bench_kernel.py pca_plda [b,n,D ...]              the per-recording PCA of PLDA scoring (xv_backend_pca.hip): one call over (b, n, D) = (256, 600, 128) and
                                                                (64, 2048, 200) at a target energy of 0.9, medians over alternated rounds, beside the float64
                                                                NumPy restatement of the same recordings on the CPU
  python tools/bench_kernel.py mfcc [utterances=256]             MFCC + energy VAD from waveforms (xv_mfcc.hip) on synthetic 16 kHz PCM, utterances of 4 - 20 s
  python tools/bench_kernel.py fbank [utterances=256]            xv_fbank (30 bins) against xv_mfcc on the same batch, alternated five times: medians and spread
  python tools/bench_kernel.py cm_encode [utterances=256]        'CM ' compression (xv_cm_encode.hip) of 400 - 2000 frames x 30 per utterance, both header forms,
                                                                against the bytes it must move and against the host writer
  python tools/bench_kernel.py augment [utterances=256] [notrace] reverberation + one background noise (xv_augment.hip) on the same synthetic PCM under impulse
                                                                responses of 4 000 / 8 000 / 16 000 taps: us per kernel role, G taps x samples / s
  python tools/bench_kernel.py resample [utterances=256]        sample-rate conversion (xv_resample.hip) of synthetic utterances of 4 - 20 s: 16000 -> 8000,
                                                                44100 -> 16000 and speed 0.9; the bare entry point and ops.resample, G fma / s, GB / s

Environment: XV_DATA_SCALE=0 (all-zero operands: DVFS check), XV_B (chunks, gemm16), ITERS (segment), XV_LIB (another build of the library).
"""
import os
import sys
import time

ROOT = os.environ.get("XV_BENCH_ROOT") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))      # XV_BENCH_ROOT: import the package of another checkout (triplet steps)
sys.path.insert(0, ROOT)
import numpy as np
import torch

rs = np.random.RandomState(0)
SCALE = float(os.environ.get("XV_DATA_SCALE", "1"))


def rnd(*s):
    return torch.from_numpy((rs.randn(*s) * SCALE).astype(np.float32)).cuda()


def timeit(fn, n=20, warm=3):
    """mean microseconds of n back-to-back calls (events on the current stream)"""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3


def bn_vectors(ops, z, rows, n):
    gamma, beta = rnd(n).abs() + 0.5, rnd(n)
    mm, mv = torch.zeros(n).cuda(), torch.ones(n).cuda()
    part = ops.col_stats(z)
    return (gamma, beta, mm, mv, part) + tuple(ops.bn_finalize(part, rows, gamma, beta, 1e-3, 0.99, 0, mm, mv, with_range=True))


def cmd_gemm(argv):
    from tf_kaldi_speaker_amd import ops
    B, T = 128, int(argv[0]) if argv else 200
    for name, t_in, c, k, o in (("tdnn2", T - 4, 512, 5, 512), ("tdnn3", T - 8, 512, 7, 512), ("tdnn4", T - 14, 512, 1, 512), ("tdnn5", T - 14, 512, 1, 1500)):
        segs = B if k > 1 else B * t_in
        tin = t_in if k > 1 else 1
        tout = tin - k + 1
        x, kern, bias = rnd(segs, tin, c), rnd(k, c, o) * 0.05, rnd(o)
        wt = ops.prep_weight_fwd(kern, c)
        wf = ops.prep_weight_dgrad(kern) if k > 1 else kern.view(c, o)
        dzp = rnd(segs * (tout + 2 * (k - 1)), o)
        fl = 2.0 * segs * tout * k * c * o
        us = timeit(lambda: ops.affine_forward(x, k, wt, bias, o, with_stats=True))
        print("%s fwd   M=%6d K=%5d N=%5d  %8.1f us  %6.1f TF" % (name, segs * tout, k * c, o, us, fl / us / 1e6))
        fl2 = 2.0 * segs * (tout + k - 1) * k * o * c
        us = timeit(lambda: ops.affine_dgrad(dzp, segs, tout, o, k, wf, c))
        print("%s dgrad M=%6d K=%5d N=%5d  %8.1f us  %6.1f TF" % (name, segs * (tout + k - 1), k * o, c, us, fl2 / us / 1e6))
        us = timeit(lambda: ops.affine_wgrad(x, k, c, dzp, tout + 2 * (k - 1), k - 1, o, kern, 1e-2))
        print("%s wgrad M=%6d N=%5d R=%6d  %8.1f us  %6.1f TF (incl. reduce)" % (name, k * c, o, segs * tout, us, fl / us / 1e6))


def cmd_gemm16(argv):
    from tf_kaldi_speaker_amd import ops
    B = int(os.environ.get("XV_B", "128"))
    T = int(argv[0]) if argv else 200
    only = argv[1].split(",") if len(argv) > 1 else None
    tot = 0.0
    for name, t_in, c, k, o in (("tdnn1", T, 32, 5, 512), ("tdnn2", T - 4, 512, 5, 512), ("tdnn3", T - 8, 512, 7, 512), ("tdnn4", T - 14, 512, 1, 512),
                                ("tdnn5", T - 14, 512, 1, 1500)):
        if only and name not in only:
            continue
        segs = B if k > 1 else B * t_in
        tin = t_in if k > 1 else 1
        tout = tin - k + 1
        x, kern, bias = rnd(segs * tin, c), rnd(k, c, o) * 0.05, rnd(o)
        xp = ops.split_planes(x)
        wtp = ops.split_planes(ops.prep_weight_fwd(kern, c))
        o_ld = (o + 7) // 8 * 8
        wf = ops.prep_weight_dgrad(kern) if k > 1 else kern.view(c, o)
        if o_ld != o:
            wf = torch.nn.functional.pad(wf.view(c, k, o), (0, o_ld - o)).reshape(c, k * o_ld).contiguous()
        wfp = ops.split_planes(wf)
        dzp = ops.split_planes(rnd(segs * (tout + 2 * (k - 1)), o))
        fl = 2.0 * segs * tout * k * c * o
        us = timeit(lambda: ops.affine_forward_f16x3(xp, segs, tin, k, wtp, bias, o, with_stats=True)); tot += us
        print("%s fwd   M=%6d K=%5d N=%5d  %8.1f us  %6.1f TF" % (name, segs * tout, k * c, o, us, fl / us / 1e6))
        if name != "tdnn1":
            fl2 = 2.0 * segs * (tout + k - 1) * k * o * c
            us = timeit(lambda: ops.affine_dgrad_f16x3(dzp, segs, tout, k, wfp, c)); tot += us
            print("%s dgrad M=%6d K=%5d N=%5d  %8.1f us  %6.1f TF" % (name, segs * (tout + k - 1), k * o_ld, c, us, fl2 / us / 1e6))
        us = timeit(lambda: ops.affine_wgrad_f16x3(xp, segs, tin, k, c, dzp, tout + 2 * (k - 1), k - 1, o, kern, 1e-2)); tot += us
        print("%s wgrad M=%6d N=%5d R=%6d  %8.1f us  %6.1f TF (incl. reduce)" % (name, k * c, o, segs * tout, us, fl / us / 1e6))
    print("sum %.1f us" % tot)


def cmd_elementwise(argv):
    """No timing of its own: 20 launches of every kernel, for a rocprofv3 kernel trace."""
    from tf_kaldi_speaker_amd import ops
    B, T = 128, (int(argv[0]) if argv else 200) - 14

    def run(fn, n=20):
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
    for n in (512, 1500):
        rows = B * T
        z, da = rnd(rows, n), rnd(rows, n)
        gamma, beta, mm, mv, part, mean, invstd, scale, shift, zmin, zmax, amax = bn_vectors(ops, z, rows, n)
        # yardstick: what a plain streaming pass (torch's vectorised element-wise kernel, out = z + 1) reaches at this footprint on this device -
        # 97.5 MB lives in the 256 MB memory-side cache between repetitions, 285.7 MB does not
        tmp = torch.empty_like(z)
        run(lambda: torch.add(z, 1.0, out=tmp))
        run(lambda: ops.col_stats(z))
        run(lambda: ops.bn_finalize(part, rows, gamma, beta, 1e-3, 0.99, 0, mm, mv))
        run(lambda: ops.bn_apply(z, scale, shift, True))
        run(lambda: ops.bn_apply_split(z, scale, shift, True, amax))
        if n == 512:
            run(lambda: ops.bn_relu_backward(da, z, B, T, gamma, mean, invstd, scale, shift, True, 4))
            run(lambda: ops.bn_relu_backward(da, z, B * T, 1, gamma, mean, invstd, scale, shift, True, 0))      # a dense layer: no padding rows (strip form)
            run(lambda: ops.bn_relu_backward_split(da, z, B, T, gamma, mean, invstd, scale, shift, zmin, zmax, True, 4))
        else:
            pool, wpos, _ = ops.stat_pool_forward_bn_aux(z, B, T, scale, shift, True)
            dpool = rnd(B, 2 * n)
            run(lambda: ops.stat_pool_forward_bn(z, B, T, scale, shift, True))
            run(lambda: ops.bn_relu_backward_pooled(pool, dpool, B, T, z, gamma, mean, invstd, scale, shift, True))
            run(lambda: ops.bn_relu_backward_pooled_aux(pool, dpool, wpos, B, T, z, gamma, mean, invstd, scale, shift, True))      # the step's form: closed-form statistics + apply
            run(lambda: ops.bn_relu_backward_pooled_split(pool, dpool, B, T, z, gamma, mean, invstd, scale, shift, zmin, zmax, True))
            # prelu (a per-channel slope + its gradient): the reduction pass has no closed form - bn_bwd_reduce_pooled_kernel<true, true, false>
            slope, dalpha = rnd(n).abs() * 0.2 + 0.01, torch.zeros(n).cuda()
            with ops.activation(slope, dalpha):
                run(lambda: ops.bn_relu_backward_pooled(pool, dpool, B, T, z, gamma, mean, invstd, scale, shift, True))
    p, g = rnd(9_830_000), rnd(9_830_000)
    run(lambda: ops.sgd_update(p, g, 0.01))
    print("done")


def cmd_width(argv):
    from tf_kaldi_speaker_amd import ops
    B, T = 128, 186
    rows = B * T
    for n in (512, 1024, 1500, 1504, 1536, 2048, 3000):
        z, da = rnd(rows, n), rnd(rows, n)
        gamma, beta, mm, mv, part, mean, invstd, scale, shift, zmin, zmax, amax = bn_vectors(ops, z, rows, n)
        tmp = torch.empty_like(z)
        t = rows * n * 4 / 1e6
        r = {}
        r["torch_add"] = (timeit(lambda: torch.add(z, 1.0, out=tmp), 30, 5), 2 * t)
        r["bn_apply"] = (timeit(lambda: ops.bn_apply(z, scale, shift, True), 30, 5), 2 * t)
        r["col_stats"] = (timeit(lambda: ops.col_stats(z), 30, 5), t)
        r["bwd_dense"] = (timeit(lambda: ops.bn_relu_backward(da, z, rows, 1, gamma, mean, invstd, scale, shift, True, 0), 30, 5), 5 * t)   # reduce (2t) + apply (3t)
        pool = ops.stat_pool_forward_bn(z, B, T, scale, shift, True)
        dpool = rnd(B, 2 * n)
        r["pool_fwd"] = (timeit(lambda: ops.stat_pool_forward_bn(z, B, T, scale, shift, True), 30, 5), t)
        r["bwd_pooled"] = (timeit(lambda: ops.bn_relu_backward_pooled(pool, dpool, B, T, z, gamma, mean, invstd, scale, shift, True), 30, 5), 2 * t)
        print(n, "  ".join("%s %.1f us %.2f TB/s" % (k, us, mb / us) for k, (us, mb) in r.items()), flush=True)


def cmd_pitch(argv):
    from tf_kaldi_speaker_amd import _lib
    from tf_kaldi_speaker_amd.ops import _s, _p
    B, T, n = 128, 186, 1500
    rows = B * T
    scale, shift = rnd(n), rnd(n)
    t = rows * n * 4 / 1e6
    for ld in (1500, 1504, 1536, 1600, 2048):
        zf = rnd(rows, ld)
        af = torch.empty_like(zf)
        part = torch.empty(4 * ((rows + 127) // 128) * n, device="cuda")
        us_a = timeit(lambda: _lib.call("xv_bn_apply", _s(), _p(zf), rows, n, ld, _p(scale), _p(shift), 1, _p(af), ld), 30, 5)
        us_b = timeit(lambda: _lib.call("xv_bn_apply", _s(), _p(zf), rows, n, ld, _p(scale), _p(shift), 1, _p(af), n), 30, 5)
        us_c = timeit(lambda: _lib.call("xv_col_stats", _s(), _p(zf), rows, n, ld, _p(part)), 30, 5)
        print("ld %d: bn_apply (out pitch ld) %.1f us %.2f TB/s | (out dense) %.1f us %.2f TB/s | col_stats %.1f us %.2f TB/s"
              % (ld, us_a, 2 * t / us_a, us_b, 2 * t / us_b, us_c, t / us_c), flush=True)


def cmd_pool(argv):
    from tf_kaldi_speaker_amd import ops
    B = 128
    T = int(argv[0]) if argv else 186
    n = int(argv[1]) if len(argv) > 1 else 1500
    z = rnd(B * T, n)
    gamma, beta, mm, mv, part, mean, invstd, scale, shift, zmin, zmax, amax = bn_vectors(ops, z, B * T, n)
    pool, wpos, _ = ops.stat_pool_forward_bn_aux(z, B, T, scale, shift, True)
    dpool = rnd(B, 2 * n)
    flush = torch.empty(300 << 18, dtype=torch.float32, device="cuda")      # 300 MB: evicts the Infinity Cache

    def timed(fn, cold, iters=30):
        tot = 0.0
        for i in range(iters + 3):
            if cold:
                flush.fill_(1.0)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record()
            torch.cuda.synchronize()
            if i >= 3:
                tot += a.elapsed_time(b)
        return tot / iters * 1e3
    mb = B * T * n * 4 / 1e6
    for name, fn, bytes_mb in (("amax (plain streaming read, for reference)", lambda: ops.amax_of(z), mb),
                               ("torch.sum (vendor streaming read)", lambda: torch.sum(z), mb),
                               ("stat_pool_forward_bn", lambda: ops.stat_pool_forward_bn(z, B, T, scale, shift, True), mb),
                               ("stat_pool_forward_bn_aux (+ wpos: the training step's form)", lambda: ops.stat_pool_forward_bn_aux(z, B, T, scale, shift, True), mb),
                               ("bn_relu_backward_pooled (reduce+finalize+apply)", lambda: ops.bn_relu_backward_pooled(pool, dpool, B, T, z, gamma, mean, invstd, scale, shift, True), 3 * mb),
                               ("bn_relu_backward_pooled_aux (closed-form statistics + apply)", lambda: ops.bn_relu_backward_pooled_aux(pool, dpool, wpos, B, T, z, gamma, mean, invstd, scale, shift, True), 2 * mb),
                               ("bn_relu_backward_pooled_split", lambda: ops.bn_relu_backward_pooled_split(pool, dpool, B, T, z, gamma, mean, invstd, scale, shift, zmin, zmax, True), 3 * mb)):
        for cold in (False, True):
            us = timed(fn, cold)
            print("%-62s %s  %7.1f us  %6.1f MB  %.2f TB/s" % (name, "cold" if cold else "warm", us, bytes_mb, bytes_mb / us))


def cmd_vlad(argv):
    """The two HBM-bound passes of GhostVLAD pooling against the statistics-pooling pass over the same [B, T, C] tensor: seven rounds, in each
    every kernel once warm (the 143 MB tensor partly in the Infinity Cache) and once cold (a 300 MB fill in front); medians over the rounds."""
    from tf_kaldi_speaker_amd import ops
    B, C = 128, 1500
    T = int(argv[0]) if argv else 186
    K = int(argv[1]) if len(argv) > 1 else 8
    G = int(argv[2]) if len(argv) > 2 else 2
    KG = K + G
    x = torch.relu(rnd(B, T, C)).contiguous()
    lim = float(np.sqrt(6.0 / (C + KG)))
    cen = torch.from_numpy(rs.uniform(-lim, lim, size=(KG, C)).astype(np.float32)).cuda()
    logits = rnd(B * T, (KG + 3) // 4 * 4)
    a = ops.vlad_softmax(logits, KG)
    r, n = ops.vlad_pool_forward(x, a, cen, K)
    dout = rnd(B, K * C)
    dr = ops.vlad_normalize_backward(r, dout, True)
    da, _ = ops.vlad_pool_backward(x, a, cen, dr)
    flush = torch.empty(300 << 18, dtype=torch.float32, device="cuda")
    mb = B * T * C * 4 / 1e6
    small = (a.numel() + r.numel() + cen.numel()) * 4 / 1e6
    kernels = [("stat_pool_forward (statistics pooling, same tensor)", lambda: ops.stat_pool_forward(x), mb),
               ("vlad_pool_forward (%d + %d clusters)" % (K, G), lambda: ops.vlad_pool_forward(x, a, cen, K), mb + small),
               ("vlad_pool_backward (d A and the value path of d x)", lambda: ops.vlad_pool_backward(x, a, cen, dr), 2 * mb + small + da.numel() * 4 / 1e6),
               ("vlad_softmax", lambda: ops.vlad_softmax(logits, KG), (logits.numel() + a.numel()) * 4 / 1e6),
               ("vlad_softmax_backward", lambda: ops.vlad_softmax_backward(a, da), (2 * a.numel() + logits.numel()) * 4 / 1e6),
               ("vlad_normalize_forward", lambda: ops.vlad_normalize_forward(r, True), 3 * r.numel() * 4 / 1e6),
               ("vlad_normalize_backward", lambda: ops.vlad_normalize_backward(r, dout, True), 5 * r.numel() * 4 / 1e6),
               ("vlad_centers_backward", lambda: ops.vlad_centers_backward(n, dr, cen, 0.01), (dr.numel() + 2 * cen.numel()) * 4 / 1e6)]

    def once(fn, cold):
        if cold:
            flush.fill_(1.0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3
    for _, fn, _ in kernels:
        for _ in range(3):
            fn()
    rounds = 7
    t = {(name, cold): [] for name, _, _ in kernels for cold in (False, True)}
    for _ in range(rounds):
        for name, fn, _ in kernels:
            for cold in (False, True):
                t[(name, cold)].append(once(fn, cold))
    print("# GhostVLAD pooling kernels, %d chunks x %d frames x %d, K = %d, G = %d; %d rounds, every kernel once warm and once cold per round;" % (B, T, C, K, G, rounds))
    print("# us = median over the rounds (min .. max), one launch between two events; MB = bytes the kernel must move")
    med = {}
    for name, _, bytes_mb in kernels:
        for cold in (False, True):
            v = sorted(t[(name, cold)])
            med[(name, cold)] = v[len(v) // 2]
            print("%-56s %s %8.1f us (%7.1f .. %7.1f) %7.1f MB %5.2f TB/s" % (name, "cold" if cold else "warm", v[len(v) // 2], v[0], v[-1], bytes_mb, bytes_mb / v[len(v) // 2]))
    base = kernels[0][0]
    for name in (kernels[1][0], kernels[2][0]):
        print("%-56s / stat_pool_forward: warm %.2f, cold %.2f" % (name, med[(name, False)] / med[(base, False)], med[(name, True)] / med[(base, True)]))
    del x, a, r, dr, da, flush, logits, dout
    torch.cuda.empty_cache()
    # the full S1 training step (128 x 200 x 30, 7 351 speakers, additive margin softmax, fp32) with either pooling, alternated on this box
    from tf_kaldi_speaker_amd import engine as E
    N = 7351
    xs = [rnd(B, T + 14, 30) for _ in range(2)]
    ys = [torch.from_numpy(rs.randint(0, N, B).astype(np.int32)).cuda() for _ in range(2)]
    configs = (("statistics_pooling", {}), ("ghost_vlad %d + %d, final l2" % (K, G), dict(pooling_type="ghost_vlad", vlad_num_centers=K, vlad_num_ghosts=G, vlad_final_l2_norm=True)))
    ms, arena = {label: [] for label, _ in configs}, {}
    for rnd_i in range(3):
        for label, kw in configs:      # one engine alive at a time (with both alive the second one's step took 7.8 ms instead of 5.7)
            eng = E.Engine(E.make_config(30, N, loss_func="additive_margin_softmax", margin_m=0.2, last_layer_linear=True, max_batch=B, max_frames=T + 14,
                                         precision="f32", **kw), device="cuda:0")
            eng.init_variables(seed=0)
            for i in range(5):
                eng.train_step(xs[i % 2], ys[i % 2], 0.01, i)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(30):
                eng.train_step(xs[i % 2], ys[i % 2], 0.01, i)
            torch.cuda.synchronize()
            ms[label].append((time.perf_counter() - t0) / 30 * 1e3)
            arena[label] = eng.arena_bytes
            eng.close()
    print("# full S1 training step, %d x %d x 30, %d speakers, fp32; 3 rounds of 30 steps per pooling, alternated (a fresh engine each time); ms / step median (min .. max)" % (B, T + 14, N))
    for label, _ in configs:
        v = sorted(ms[label])
        print("%-40s %.3f ms (%.3f .. %.3f)   arena %.0f MB" % (label, v[1], v[0], v[-1], arena[label] / 1e6))


def triplet_steps(argv):
    """triplet step <head>: ms / step of 30 S1-shaped training steps (128 x 200 x 30, fp32, SGD) in this process, with the library $XV_LIB names -
    head = softmax (AM-Softmax m = 0.2 over 7 351 speakers, the benchmark's step) | angular (angular_triplet_loss, "all" mining, additive margin
    0.1, 64 speakers x 2 segments) | semihard.   triplet steps <checkout of the parent commit, library built> [rounds=5]: those runs as fresh
    processes, alternated: the parent's softmax step (its package and library, through $XV_BENCH_ROOT), this tree's softmax step, this tree's
    pairwise steps; medians and spreads."""
    import subprocess
    if argv[0] == "step":
        from tf_kaldi_speaker_amd import engine as E
        B, T, head = 128, 200, argv[1]
        kw = dict(loss_func="additive_margin_softmax", margin_m=0.2) if head == "softmax" else (
            dict(loss_func="angular_triplet_loss", margin=0.1, triplet_type="all", loss_type="additive_margin_softmax") if head == "angular" else
            dict(loss_func="ge2e_loss", ge2e_loss_type=head[5:], num_speakers_per_batch=B // 2, num_segments_per_speaker=2) if head.startswith("ge2e_") else
            dict(loss_func="semihard_triplet_loss", margin=0.2, feature_norm=True, feature_scaling_factor=1.0))
        eng = E.Engine(E.make_config(30, 7351, last_layer_linear=True, max_batch=B, max_frames=T, precision="f32", **kw), device="cuda:0")
        eng.init_variables(seed=0)
        xs = [rnd(B, T, 30) for _ in range(2)]
        ys = [torch.from_numpy((rs.randint(0, 7351, B) if head == "softmax" else np.repeat(rs.permutation(7351)[:B // 2], 2)).astype(np.int32)).cuda() for _ in range(2)]
        for i in range(5):
            eng.train_step(xs[i % 2], ys[i % 2], 0.01, i)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(30):
            eng.train_step(xs[i % 2], ys[i % 2], 0.01, i)
        torch.cuda.synchronize()
        print("STEP_MS %s %.4f" % (head, (time.perf_counter() - t0) / 30 * 1e3))
        eng.close()
        return
    parent, rounds = os.path.abspath(argv[1]), int(argv[2]) if len(argv) > 2 else 5
    runs = [("parent commit, AM-Softmax", "softmax", parent), ("this tree, AM-Softmax", "softmax", None), ("this tree, angular_triplet_loss", "angular", None),
            ("this tree, semihard_triplet_loss", "semihard", None)]
    if argv[0] == "ge2e-steps":      # ge2e steps <parent tree> [rounds]: the GE2E step (64 speakers x 2 segments) against the parent's angular-triplet step
        runs = [("parent commit, angular_triplet_loss", "angular", parent), ("this tree, ge2e_loss softmax", "ge2e_softmax", None),
                ("this tree, ge2e_loss contrastive", "ge2e_contrastive", None)]
    ms = {label: [] for label, _, _ in runs}
    for _ in range(rounds):
        for label, head, lib in runs:
            env = dict(os.environ)
            env.pop("XV_BENCH_ROOT", None)
            if lib:
                env["XV_BENCH_ROOT"] = lib
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "triplet", "step", head], env=env, capture_output=True, text=True, timeout=240)
            line = [l for l in out.stdout.split("\n") if l.startswith("STEP_MS")]
            if out.returncode != 0 or not line:
                sys.exit("step run failed (%s): %s" % (label, out.stderr[-2000:]))
            ms[label].append(float(line[0].split()[2]))
    print("# S1-shaped training step, 128 x 200 x 30, fp32, SGD: 30 steps after 5 in a fresh process per figure, %d alternated rounds; ms / step" % rounds)
    for label, _, _ in runs:
        v = sorted(ms[label])
        print("%-36s median %.3f  (%.3f .. %.3f)  spread %.3f   %s" % (label, v[len(v) // 2], v[0], v[-1], v[-1] - v[0], " ".join("%.3f" % x for x in ms[label])), flush=True)


def cmd_triplet(argv):
    """Forward (G = X X^T, the row scan, the final sum: 3 launches) and backward (symmetrise, d X = A X: 2 launches) of each pairwise head, and
    the e2e validation loss (4 launches), as the ops launch them: seven rounds, in each every call once warm and once cold (a 300 MB fill in
    front); medians over the rounds."""
    if argv and argv[0] in ("step", "steps"):
        return triplet_steps(argv)
    from tf_kaldi_speaker_amd import ops
    flush = torch.empty(300 << 18, dtype=torch.float32, device="cuda")
    heads = [("semihard", ops.pair_loss_config("semihard_triplet_loss", margin=0.2)),
             ("semihard squared", ops.pair_loss_config("semihard_triplet_loss", margin=0.2, squared=True)),
             ("angular all am 0.1", ops.pair_loss_config("angular_triplet_loss", margin=0.1, triplet_type="all")),
             ("angular all arc 0.3", ops.pair_loss_config("angular_triplet_loss", margin=0.3, triplet_type="all", loss_type="additive_angular_margin_softmax")),
             ("angular all asoftmax 4", ops.pair_loss_config("angular_triplet_loss", margin=4, triplet_type="all", loss_type="asoftmax")),
             ("angular hard am 0.1", ops.pair_loss_config("angular_triplet_loss", margin=0.1, triplet_type="hard"))]

    def once(fn, cold):
        if cold:
            flush.fill_(1.0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3
    rounds = 7
    print("# pairwise loss heads, D = 512; %d rounds, every call once warm and once cold per round; us = median over the rounds (min .. max)," % rounds)
    print("# between two events around the op (forward: 3 launches, backward: 2, e2e: 4; the ops' own allocations of loss / stats / dx included)")
    for n_spk, n_seg in ((64, 10), (128, 1), (32, 4)):
        b = n_spk * n_seg
        x = rnd(b, 512) + 0.5 * rnd(n_spk, 512).repeat_interleave(n_seg, dim=0)
        xu = (x / x.norm(dim=1, keepdim=True)).contiguous()
        y = torch.arange(n_spk, dtype=torch.int32, device="cuda").repeat_interleave(n_seg).contiguous()
        calls = []
        for name, cfg in heads:
            xin = xu if name.startswith("semihard") else x
            _, _, ws = ops.pair_loss(cfg, xin, y)
            dx = torch.empty_like(xin)
            calls.append((name + " forward", lambda cfg=cfg, xin=xin, ws=ws: ops.pair_loss(cfg, xin, y, ws=ws)))
            calls.append((name + " backward", lambda cfg=cfg, xin=xin, ws=ws, dx=dx: ops.pair_loss_backward(cfg, xin, y, ws, out=dx)))
        ws2 = torch.empty_like(ws)
        calls.append(("e2e_valid_loss", lambda: ops.e2e_valid_loss(x, n_spk, n_seg, ws=ws2)))
        for _, fn in calls:
            for _ in range(3):
                fn()
        t = {(name, cold): [] for name, _ in calls for cold in (False, True)}
        for _ in range(rounds):
            for name, fn in calls:
                for cold in (False, True):
                    t[(name, cold)].append(once(fn, cold))
        print("%d speakers x %d segments x 512 (B = %d)" % (n_spk, n_seg, b))
        for name, _ in calls:
            for cold in (False, True):
                v = sorted(t[(name, cold)])
                print("  %-36s %s %8.1f us (%7.1f .. %7.1f)" % (name, "cold" if cold else "warm", v[len(v) // 2], v[0], v[-1]), flush=True)


def cmd_ge2e(argv):
    """Forward (G = X X^T, the speaker norms, the row kernel, the final sum: 4 launches) and backward (Q, symmetrise, d X = A X, two scalar copies:
    5 launches) of the GE2E training loss in both types, beside the angular "all" head's forward and the pairwise backward on the same rows:
    seven rounds, in each every call once warm and once cold (a 300 MB fill in front); medians over the rounds.
    ge2e steps <checkout of the parent commit, library built> [rounds=5]: the S1-shaped step with this head against the parent's angular step."""
    if argv and argv[0] == "steps":
        return triplet_steps(["ge2e-steps"] + argv[1:])
    from tf_kaldi_speaker_amd import ops
    flush = torch.empty(300 << 18, dtype=torch.float32, device="cuda")

    def once(fn, cold):
        if cold:
            flush.fill_(1.0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3
    rounds = 7
    print("# GE2E training loss, D = 512, w = 10, b = -5; %d rounds, every call once warm and once cold per round; us = median over the rounds (min .. max)," % rounds)
    print("# between two events around the op (the ops' own allocations of loss / stats / dx / dw / db included)")
    w, b = torch.tensor([10.0], device="cuda"), torch.tensor([-5.0], device="cuda")
    angular = ops.pair_loss_config("angular_triplet_loss", margin=0.1, triplet_type="all")
    for n_spk, n_seg in ((64, 10), (32, 4)):
        x = rnd(n_spk * n_seg, 512) + 0.5 * rnd(n_spk, 512).repeat_interleave(n_seg, dim=0)
        y = torch.arange(n_spk, dtype=torch.int32, device="cuda").repeat_interleave(n_seg).contiguous()
        dx = torch.empty_like(x)
        calls = []
        for name in ("softmax", "contrastive"):
            cfg = ops.ge2e_loss_config(name, n_spk, n_seg)
            _, _, ws = ops.ge2e_loss(cfg, x, w, b)
            calls.append(("ge2e %s forward" % name, lambda cfg=cfg, ws=ws: ops.ge2e_loss(cfg, x, w, b, ws=ws)))
            calls.append(("ge2e %s backward" % name, lambda cfg=cfg, ws=ws: ops.ge2e_loss_backward(cfg, x, w, b, ws, out=dx)))
        _, _, wsa = ops.pair_loss(angular, x, y)
        calls.append(("angular all am 0.1 forward", lambda: ops.pair_loss(angular, x, y, ws=wsa)))
        calls.append(("angular all am 0.1 backward", lambda: ops.pair_loss_backward(angular, x, y, wsa, out=dx)))
        for _, fn in calls:
            for _ in range(3):
                fn()
        t = {(name, cold): [] for name, _ in calls for cold in (False, True)}
        for _ in range(rounds):
            for name, fn in calls:
                for cold in (False, True):
                    t[(name, cold)].append(once(fn, cold))
        print("%d speakers x %d segments x 512 (B = %d)" % (n_spk, n_seg, n_spk * n_seg))
        for name, _ in calls:
            for cold in (False, True):
                v = sorted(t[(name, cold)])
                print("  %-36s %s %8.1f us (%7.1f .. %7.1f)" % (name, "cold" if cold else "warm", v[len(v) // 2], v[0], v[-1]), flush=True)


def cmd_segment(argv):
    from tf_kaldi_speaker_amd import ops
    iters = int(os.environ.get("ITERS", "200"))
    for name, m, n, k in (("tdnn6 fwd", 128, 512, 3000), ("tdnn7 fwd", 128, 512, 512), ("logits", 128, 7351, 512), ("d out", 128, 512, 7352),
                          ("d tdnn7", 128, 512, 512), ("d pool", 128, 3000, 512)):
        x = rnd(m, k)
        wt = rnd(n, k) / float(np.sqrt(k))
        bias = torch.zeros(n).cuda()
        t_sk = timeit(lambda: ops.segment_gemm(x, wt, bias), iters, 10)
        x3 = x.view(m, 1, k)
        t_nt = timeit(lambda: ops.affine_forward(x3, 1, wt, bias, n), iters, 10)
        print("%-10s M=%d N=%5d K=%5d  segment_gemm %6.1f us   affine_forward (2 launches) %6.1f us" % (name, m, n, k, t_sk, t_nt))


def cmd_staged(argv):
    from tf_kaldi_speaker_amd import engine as E
    from tf_kaldi_speaker_amd.parallel import GradAllReduce
    B, T, D, N = 128, 200, 30, 7351
    eng = E.Engine(E.make_config(D, N, loss_func="additive_margin_softmax", margin_m=0.2, last_layer_linear=True, max_batch=B, max_frames=T), device="cuda:0")
    eng.init_variables(seed=0)
    x = rnd(B, T, D)
    y = torch.from_numpy(rs.randint(0, N, B).astype(np.int32)).cuda()

    def run(ar, n=40):
        for i in range(5):
            eng.train_step(x, y, 0.01, i, allreduce=ar)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(n):
            eng.train_step(x, y, 0.01, i, allreduce=ar)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3
    for _ in range(2):
        print("plain  %.4f ms" % run(None))
        print("staged %.4f ms (4 stages, no collective)" % run(GradAllReduce(None, 1)))
    import torch.distributed as dist
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29531")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    for _ in range(2):
        print("staged + one-rank RCCL all-reduce on the comm stream %.4f ms" % run(GradAllReduce(dist, 1, always=True)))
    dist.destroy_process_group()


def cmd_score(argv):
    """Time per op of the scoring stage; the trial kernel's traffic against the 8 TB/s HBM peak (2 rows of d floats, two indices and one score
    per trial - a flat streaming kernel reaches 0.82 of the peak here); the cohort op's GEMM launches alone (the same
    row tiles through xv_affine_forward without scratch, as xv_score_cohort_stats runs them) against the whole op: the rest is the selection."""
    import ctypes as C
    from tf_kaldi_speaker_amd import _lib, ops
    from tf_kaldi_speaker_amd.ops import _p, _s
    d, ws_bytes = 512, 1 << 30
    sizes = {"small": ("VoxCeleb1-O-sized", 4708, 37720, 2000, 200), "large": ("VoxCeleb1-E-sized", 145160, 581480, 6000, 300)}
    for key in (argv or ["small", "large"]):
        name, n, m, n_cohort, top_k = sizes[key]
        raw, craw = rnd(n, d), rnd(n_cohort, d)
        x, cohort = ops.score_prepare(raw), ops.score_prepare(craw)
        ei, ti = rs.randint(0, n, m), rs.randint(0, n, m)
        print("%s: %d vectors, %d trials, cohort %d, top-k %d, d = %d" % (name, n, m, n_cohort, top_k, d), flush=True)
        us = timeit(lambda: ops.score_prepare(raw, out=x), 10, 2)
        print("  prepare                 %9.1f us  %.2f TB/s (one read, one write)" % (us, 2.0 * n * d * 4 / us / 1e6), flush=True)
        ei_d, ti_d = torch.from_numpy(ei.astype(np.int32)).cuda(), torch.from_numpy(ti.astype(np.int32)).cuda()
        out = torch.empty(m, device="cuda")
        stats = ops.score_cohort_stats(x, cohort, d, top_k, ws_bytes=ws_bytes)
        for label, st in (("trials (raw)", None), ("trials (AS-norm)", stats)):
            us = timeit(lambda: _lib.call("xv_score_trials", _s(), _p(x), d, n, _p(x), d, n, d, _p(ei_d), _p(ti_d), C.c_int64(m), _p(st), _p(st), _p(out)),
                        10, 2)
            mb = m * (2.0 * d * 4 + 12 + (16 if st is not None else 0)) / 1e6
            print("  %-22s  %9.1f us  %.2f TB/s = %.2f of the 8 TB/s peak (gathered rows; the tables are %.0f MB)" % (label, us, mb / us, mb / us / 8.0, n * d * 4 / 1e6),
                  flush=True)
        ws = torch.empty(ws_bytes // 4, device="cuda")
        ldn = (n_cohort + 3) // 4 * 4
        tile = min((n + 127) // 128 * 128, ws_bytes // (ldn * 4) // 128 * 128)

        def whole():
            _lib.call("xv_score_cohort_stats", _s(), _p(x), d, n, _p(cohort), d, n_cohort, d, top_k, _p(stats), _p(ws), C.c_size_t(ws_bytes))

        def gemms():
            for r0 in range(0, n, tile):
                rows = min(tile, n - r0)
                _lib.call("xv_affine_forward", _s(), _p(x[r0:]), rows, 1, d, 1, _p(cohort), None, _p(ws), n_cohort, ldn, None, None, C.c_size_t(0))
        us_all, us_gemm = timeit(whole, 5, 1), timeit(gemms, 5, 1)
        fl = 2.0 * n * n_cohort * d
        print("  cohort statistics       %9.1f us in %d row tile(s) of %d: GEMM %.1f us (%.1f TF) = %.2f of the op, selection %.1f us = %.2f"
              % (us_all, (n + tile - 1) // tile, tile, us_gemm, fl / us_gemm / 1e6, us_gemm / us_all, us_all - us_gemm, 1.0 - us_gemm / us_all), flush=True)


def cmd_backend(argv):
    """Time per device op of the LDA / PLDA back end: scatter (the TN GEMM's FLOPs against the whole op: the rest is the centred copy and the
    slab sums), per-speaker means (gathered rows against the 8 TB/s peak), PLDA normalisation (one read, one write) and the trial kernel
    (2 rows of dim floats, the coefficient rows, three indices and one score per trial)."""
    from tf_kaldi_speaker_amd import ops
    from tf_kaldi_speaker_amd.misc import backend as B
    d, dim = 512, 200
    sizes = {"small": ("VoxCeleb1-sized", 148642, 1211, 37720), "large": ("VoxCeleb2-dev-sized", 1092009, 5994, 581480)}
    for key in (argv or ["small", "large"]):
        name, n, speakers, m = sizes[key]
        x, mean = rnd(n, d), rnd(d)
        print("%s: %d vectors of %d speakers, %d trials, d = %d, dim = %d" % (name, n, speakers, m, d, dim), flush=True)
        us = timeit(lambda: ops.backend_scatter(x, mean=mean), 5, 1)
        print("  scatter (centred)       %9.1f us  %.1f TF (2 n d^2)" % (us, 2.0 * n * d * d / us / 1e6), flush=True)
        offsets = np.linspace(0, n, speakers + 1).astype(np.int64)
        rows = rs.permutation(n)
        us = timeit(lambda: ops.backend_group_means(x, d, offsets, rows), 5, 1)
        print("  group means             %9.1f us  %.2f TB/s (gathered rows; includes the index upload)" % (us, n * d * 4.0 / us / 1e6), flush=True)
        psi = np.sort(rs.uniform(0.05, 5.0, dim))[::-1].copy()
        u, psi_d = rnd(n, dim), torch.from_numpy(psi.astype(np.float32)).cuda()
        out = torch.empty_like(u)
        us = timeit(lambda: ops.backend_plda_normalize(u, dim, psi_d, out=out), 10, 2)
        print("  plda_normalize          %9.1f us  %.2f TB/s (one read, one write)" % (us, 2.0 * n * dim * 4 / us / 1e6), flush=True)
        n_e = rs.choice([1, 3, 8], n)
        distinct, nidx = np.unique(n_e, return_inverse=True)
        coef, g, k0 = (torch.from_numpy(a).cuda() for a in B.plda_coefficients(psi, distinct))
        ei, ti = rs.randint(0, n, m), rs.randint(0, n, m)
        us = timeit(lambda: ops.backend_plda_trials(out, out, dim, ei, ti, nidx, coef, g, k0), 5, 1)
        mb = m * (2.0 * dim * 4 + 16) / 1e6
        print("  plda_trials             %9.1f us  %.2f TB/s of gathered rows (includes the index checks and uploads of ops.py)" % (us, mb / us), flush=True)


def cmd_plda_cohort(argv):
    """Time of the cohort statistics of PLDA scores (xv_backend_plda_cohort_stats, d = 200, 4 k rows with the counts 1 / 3 / 8 mixed) against
    cohorts of 4 k and 40 k rows; the op's GEMM launches alone (the same row tiles through xv_affine_forward without scratch) against the
    whole op: the rest is the column-term and fold kernels and the selection."""
    import ctypes as C
    from tf_kaldi_speaker_amd import _lib, ops
    from tf_kaldi_speaker_amd.misc import backend as B
    from tf_kaldi_speaker_amd.ops import _p, _s
    d, n, top_k = 200, 4096, 300
    psi = np.sort(rs.uniform(0.05, 5.0, d))[::-1].copy()
    coef, g, k0 = (torch.from_numpy(a).cuda() for a in B.plda_coefficients(psi, [1, 3, 8]))
    nidx = torch.from_numpy(rs.randint(0, 3, n).astype(np.int32)).cuda()
    x = rnd(n, d)
    sizes = {"small": 4096, "large": 40960}
    for key in (argv or ["small", "large"]):
        n_cohort = sizes[key]
        cohort = rnd(n_cohort, d)
        ws_bytes = ops.backend_plda_cohort_workspace_bytes(n, n_cohort, d, 3)
        ws = torch.empty(ws_bytes // 4, device="cuda")
        stats = torch.empty((n, 2), device="cuda")
        ldn = (n_cohort + 3) // 4 * 4
        print("plda_cohort: %d rows, cohort %d, top-k %d, d = %d, 3 counts, workspace %.0f MB" % (n, n_cohort, top_k, d, ws_bytes / 1e6), flush=True)

        def whole():
            _lib.call("xv_backend_plda_cohort_stats", _s(), _p(x), d, n, _p(nidx), _p(cohort), d, n_cohort, d, _p(coef), d, 3, _p(g), _p(k0), top_k,
                      _p(stats), _p(ws), C.c_size_t(ws_bytes))

        def gemm():
            _lib.call("xv_affine_forward", _s(), _p(x), n, 1, d, 1, _p(cohort), None, _p(ws), n_cohort, ldn, None, None, C.c_size_t(0))
        us_all, us_gemm = timeit(whole, 5, 1), timeit(gemm, 5, 1)
        fl = 2.0 * n * n_cohort * d
        print("  cohort statistics       %9.1f us: GEMM %.1f us (%.1f TF) = %.2f of the op, column terms + fold + selection %.1f us = %.2f"
              % (us_all, us_gemm, fl / us_gemm / 1e6, us_gemm / us_all, us_all - us_gemm, 1.0 - us_gemm / us_all), flush=True)


def cmd_dense(argv):
    """Time of the dense score matrix of one recording at d = 200: xv_score_dense (one GEMM launch) and xv_backend_plda_dense (column terms,
    fold, the GEMM, the finishing kernel), written into a view of a packed buffer as misc/diarization.py does; five alternated rounds."""
    from tf_kaldi_speaker_amd import ops
    from tf_kaldi_speaker_amd.misc import backend as B
    d = 200
    psi = np.sort(rs.uniform(0.05, 5.0, d))[::-1].copy()
    tabs = tuple(torch.from_numpy(a).cuda() for a in B.plda_coefficients(psi, [1]))
    sizes = [int(a) for a in argv] or [200, 800, 2000]
    xs = {n: ops.score_prepare(rnd(n, d)) for n in sizes}
    views = {n: torch.empty(8 + n * ((n + 3) // 4 * 4), device="cuda")[8:].view(n, (n + 3) // 4 * 4)[:, :n] for n in sizes}
    times = {(n, k): [] for n in sizes for k in ("cos", "plda")}
    for _ in range(5):
        for n in sizes:
            times[(n, "cos")].append(timeit(lambda: ops.score_dense(xs[n], d, out=views[n]), 20, 3))
            times[(n, "plda")].append(timeit(lambda: ops.backend_plda_dense(xs[n], d, *tabs, out=views[n]), 20, 3))
    for n in sizes:
        cos, plda = np.median(times[(n, "cos")]), np.median(times[(n, "plda")])
        print("dense: n = %4d, d = %d: score_dense %8.1f us (%.2f TF; rounds %s), backend_plda_dense %8.1f us (rounds %s)"
              % (n, d, cos, 2.0 * n * n * d / cos / 1e6, " ".join("%.1f" % t for t in times[(n, "cos")]), plda,
                 " ".join("%.1f" % t for t in times[(n, "plda")])), flush=True)


def _scipy_average_linkage(s):      # (module level: the pool's workers import it)
    from scipy.cluster.hierarchy import linkage
    n = s.shape[0]
    return linkage(-s.astype(np.float64)[np.triu_indices(n, 1)], "average")[:, 2].sum()


def cmd_ahc(argv):
    """One xv_ahc_cluster call over `recordings` score matrices of n windows each (cosines of clustered unit vectors, 4 speakers), merged down
    to one cluster: milliseconds per call, medians over five rounds that alternate the sizes.  Beside it scipy.cluster.hierarchy.linkage
    (-S, "average") over the same matrices on 16 worker processes - started and joined BEFORE this process opens the GPU, so that no child
    holds it."""
    import multiprocessing as mp
    from tf_kaldi_speaker_amd import ops
    recordings = int(argv[0]) if argv else 64
    sizes = [int(a) for a in argv[1:]] or [200, 800, 2000]
    host = {}
    for n in sizes:
        mats = []
        for _ in range(recordings):
            x = rs.randn(4, 64)[rs.randint(0, 4, n)] + 0.6 * rs.randn(n, 64)
            x /= np.linalg.norm(x, axis=1, keepdims=True)
            mats.append((x @ x.T).astype(np.float32))
        host[n] = mats
    cpu = {}
    with mp.get_context("spawn").Pool(16) as pool:
        pool.map(_scipy_average_linkage, host[sizes[0]][:16])      # the workers have imported scipy
        for n in sizes:
            t0 = time.time()
            pool.map(_scipy_average_linkage, host[n], chunksize=1)
            cpu[n] = (time.time() - t0) * 1e3
    dev = {}
    for n in sizes:
        ld = (n + 3) // 4 * 4
        buf = torch.zeros(recordings * n * ld, device="cuda")
        for i, m in enumerate(host[n]):
            buf[i * n * ld:(i + 1) * n * ld].view(n, ld)[:, :n] = torch.from_numpy(m).cuda()
        dev[n] = (buf, np.arange(recordings, dtype=np.int64) * n * ld, np.full(recordings, n, np.int32), np.full(recordings, ld, np.int32),
                  np.ones(recordings, np.int32))
    times = {n: [] for n in sizes}
    for _ in range(5):
        for n in sizes:
            buf, off, nn, ld, tg = dev[n]
            times[n].append(timeit(lambda: ops.ahc_cluster(buf, off, nn, ld, targets=tg), 2, 1) / 1e3)
    for n in sizes:
        med = float(np.median(times[n]))
        print("ahc: %d recordings x n = %4d, %d merges each: %9.2f ms per call (rounds %s) = %.2f us per merge step of a recording's workgroup; "
              "scipy average linkage, 16 processes, the same matrices: %9.1f ms"
              % (recordings, n, n - 1, med, " ".join("%.2f" % t for t in times[n]), med * 1e3 / (n - 1), cpu[n]), flush=True)


def cmd_ahc2(argv):
    """Two-pass clustering of ONE long recording (ops.ahc_cluster_two_pass, first_pass_max_points 2048, down to 4 speakers) at n = 4096 and
    8192 windows, and the single pass (ops.ahc_cluster) over the first 2048 windows for scale: milliseconds per call, medians over five
    rounds that alternate the sizes.  The stages apart: the first pass (ops.ahc_cluster_from over the subsets), the cluster sums (the bare
    xv_ahc_cluster_sums entry on uploaded lists: its three launches and nothing else) and the seeded second pass on a fresh copy of the
    seed.  Beside the sums: torch.sum over the recording's n x ld floats (a flat streaming read of the same matrix) and n^2 x 4 bytes at
    0.82 of the 8 TB/s HBM peak (what DESIGN.md section 8 quotes for a flat streaming kernel)."""
    import ctypes as C
    from tf_kaldi_speaker_amd import _lib, ops
    from tf_kaldi_speaker_amd._host import _p, _s, upload
    sizes = [int(a) for a in argv] or [4096, 8192]
    speakers, cap, inf = 4, 2048, float("-inf")
    data = {}
    for n in sizes + [cap]:
        x = rs.randn(speakers, 64)[rs.randint(0, speakers, n)] + 0.6 * rs.randn(n, 64)
        x /= np.linalg.norm(x, axis=1, keepdims=True)
        xd = torch.from_numpy(x.astype(np.float32)).cuda()
        ld = (n + 3) // 4 * 4
        buf = torch.zeros(n * ld, device="cuda")
        buf.view(n, ld)[:, :n] = xd @ xd.T
        data[n] = (buf, ld)
    stages = {}
    for n in sizes:      # the stages' inputs, as ops.ahc_cluster_two_pass builds them
        buf, ld = data[n]
        bounds = ops.ahc_subsets(n, cap)
        rows = np.diff(bounds)
        first = (buf, bounds[:-1] * (ld + 1), rows, np.full(rows.size, ld), np.minimum(rows, 10 * speakers))
        local = ops.ahc_cluster_from(*first[:4], floors=first[4], threshold=inf)[0].cpu().numpy().astype(np.int64)
        clusters = np.concatenate([local[a:b] + 10 * speakers * k for k, (a, b) in enumerate(zip(bounds[:-1], bounds[1:]))])
        members, starts, c = ops.ahc_member_lists(clusters, [n])
        seed, dsizes = ops.ahc_cluster_sums(buf, [0], [n], [ld], members, starts, c)
        cc = int(c[0])
        dev = dict(off=upload([0], np.int64, "cuda"), n=upload([n], np.int32, "cuda"), ld=upload([ld], np.int32, "cuda"), c=upload(c, np.int32, "cuda"),
                   members=upload(members, np.int32, "cuda"), starts=upload(starts, np.int32, "cuda"), seed=torch.empty_like(seed),
                   sizes=torch.empty_like(dsizes), status=torch.empty(1, dtype=torch.int32, device="cuda"))
        ws_bytes = ops.ahc_cluster_sums_workspace_bytes([n], c)
        dev["ws"] = torch.empty(ws_bytes // 8, dtype=torch.float64, device="cuda")
        bare = lambda buf=buf, n=n, cc=cc, d=dev, ws_bytes=ws_bytes: _lib.call(
            "xv_ahc_cluster_sums", _s(), _p(buf), C.c_int64(buf.numel()), _p(d["off"]), _p(d["n"]), _p(d["ld"]), _p(d["c"]), _p(d["members"]), _p(d["starts"]),
            1, n, cc, C.c_int64(n), C.c_int64(cc), C.c_int64(cc * cc), C.c_int64(n * cc), _p(d["seed"]), _p(d["sizes"]), _p(d["status"]), _p(d["ws"]),
            C.c_size_t(ws_bytes))
        bare()
        assert int(dev["status"][0]) == 0 and torch.equal(dev["seed"], seed)
        stages[n] = (first, bare, seed, dsizes.cpu().numpy(), cc, dev)
    times = {}
    for _ in range(5):
        for n in sizes:
            buf, ld = data[n]
            first, bare, seed, hsizes, cc, dev = stages[n]
            t = times.setdefault(n, {k: [] for k in ("two_pass", "first", "sums", "second", "stream")})
            t["two_pass"].append(timeit(lambda: ops.ahc_cluster_two_pass(buf, [0], [n], [ld], targets=[speakers], first_pass_max_points=cap), 3, 1) / 1e3)
            t["first"].append(timeit(lambda: ops.ahc_cluster_from(*first[:4], floors=first[4], threshold=inf), 3, 1) / 1e3)
            t["sums"].append(timeit(bare, 20, 3) / 1e3)
            t["second"].append(timeit(lambda: ops.ahc_cluster_from(None, None, [cc], floors=[speakers], seed=seed.clone(), sizes=hsizes), 5, 1) / 1e3)
            t["stream"].append(timeit(lambda: buf.sum(), 20, 3) / 1e3)
        buf, ld = data[cap]
        times.setdefault(cap, {"single": []})["single"].append(timeit(lambda: ops.ahc_cluster(buf, [0], [cap], [ld], targets=[speakers]), 3, 1) / 1e3)
    show = lambda v: "%9.3f ms (rounds %s)" % (float(np.median(v)), " ".join("%.3f" % a for a in v))
    print("ahc2: single pass, n = %d down to %d clusters: %s" % (cap, speakers, show(times[cap]["single"])), flush=True)
    for n in sizes:
        t, cc = times[n], stages[n][4]
        sums, bound = float(np.median(t["sums"])), 4.0 * n * n / (0.82 * 8e12) * 1e3
        print("ahc2: n = %5d, %d subsets, %d survivors, down to %d clusters: two passes %s" % (n, len(ops.ahc_subsets(n, cap)) - 1, cc, speakers, show(t["two_pass"])))
        print("ahc2: n = %5d   first pass %s" % (n, show(t["first"])))
        print("ahc2: n = %5d   cluster sums, bare entry %s" % (n, show(t["sums"])))
        print("ahc2: n = %5d   second pass, seeded (with the copy of the %d x %d seed) %s" % (n, cc, cc, show(t["second"])))
        print("ahc2: n = %5d   torch.sum over the matrix's %d floats %s" % (n, data[n][0].numel(), show(t["stream"])))
        print("ahc2: n = %5d   n^2 floats at 0.82 of 8 TB/s: %.4f ms; the cluster sums take %.1f x that, %.2f x the torch.sum" %
              (n, bound, sums / bound, sums / float(np.median(t["stream"]))), flush=True)


def cmd_diar_tune(argv):
    """Threshold tuning over `recordings` synthetic recordings of n windows in 128 dimensions (4 speakers, cosine scores) at 13 thresholds.
    The sweep side: Diarizer.sweep (one clustering, xv_ahc_cut) + DerSweep (its set-up, then xv_diar_confusion and the assignments).  The
    baseline side, the only route without them: 13 x (Diarizer.cluster + rttm_turns + der() per recording).  Host clock around each side,
    ending in a device synchronise; five rounds that alternate the two sides, medians with min .. max; the sweep's parts apart; the two
    ops alone (events, 20 calls back to back).  collar 0 and overlap "first" are der()'s rules: the two sides must give the same DER."""
    from tf_kaldi_speaker_amd import ops
    from tf_kaldi_speaker_amd.misc import diarization as D
    from tf_kaldi_speaker_amd.misc import scoring as S
    recordings = int(argv[0]) if argv else 64
    n = int(argv[1]) if len(argv) > 1 else 600
    thresholds = [float(t) for t in np.linspace(0.0, 0.6, 13)]
    windows = [(0.01 * s, 0.01 * e) for s, e in D.subsegments(0, 75 * (n + 1), 150, 75, 50)]
    emb, reference, subsegs = {}, {}, {}
    for i in range(recordings):
        who = np.repeat(rs.randint(0, 4, n // 8 + 1), 8)[:n]      # turns of eight windows
        x = rs.randn(4, 128)[who] + 0.6 * rs.randn(n, 128)
        key = "rec%03d" % i
        emb[key], subsegs[key] = x.astype(np.float32), windows
        reference[key] = [(s, e, "spk%d" % l) for s, e, l in D.rttm_turns(windows, who)]
    scorer = S.CosineScorer("cuda:0")

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.time()
        out = fn()
        torch.cuda.synchronize()
        return (time.time() - t0) * 1e3, out

    def sweep_side():
        parts = {}
        parts["sweep"], labels = clock(lambda: D.Diarizer(scorer, threshold=0.0).sweep(emb, thresholds))
        parts["set-up"], der = clock(lambda: D.DerSweep("cuda:0", reference, subsegs, collar=0.0, overlap="first"))
        parts["score"], table = clock(lambda: der.score(labels))
        return parts, [table.pooled(k)[3] if table.pooled(k) else float("nan") for k in range(len(thresholds))]      # (NaN: a cut of more than 256 clusters)

    def baseline_side():
        ders = []
        for t in thresholds:
            labels = D.Diarizer(scorer, threshold=t).cluster(emb)
            counts = np.zeros(2)
            for key in emb:
                turns = D.rttm_turns(windows, labels[key])
                speech = sum(int(round(e / D.DER_FRAME)) - int(round(s / D.DER_FRAME)) for s, e, _ in reference[key])      # (its turns do not overlap)
                counts += speech * D.der(reference[key], turns)[3], speech
            ders.append(counts[0] / counts[1])
        return ders

    sweep_side(), baseline_side()      # warm
    times = {"sweep side": [], "baseline side": [], "sweep": [], "set-up": [], "score": []}
    for _ in range(5):
        ms, (parts, swept) = clock(sweep_side)
        times["sweep side"].append(ms)
        for k, v in parts.items():
            times[k].append(v)
        ms, base = clock(baseline_side)
        times["baseline side"].append(ms)
        assert np.allclose(np.where(np.isnan(swept), base, swept), base, rtol=0, atol=1e-12), (swept, base)
    show = lambda v: "%9.2f ms (min %.2f .. max %.2f)" % (float(np.median(v)), min(v), max(v))
    print("diar_tune: %d recordings x %d windows x 128, %d thresholds, cosine; pooled DER per threshold %s" % (recordings, n, len(thresholds), " ".join("%.4f" % d for d in swept)))
    print("diar_tune: sweep side (Diarizer.sweep + DerSweep)                 %s" % show(times["sweep side"]))
    print("diar_tune: baseline side (%d x (Diarizer.cluster + rttm_turns + der)) %s" % (len(thresholds), show(times["baseline side"])))
    print("diar_tune: the baseline takes %.2f x the sweep (medians)" % (float(np.median(times["baseline side"])) / float(np.median(times["sweep side"]))))
    for k, what in (("sweep", "Diarizer.sweep: scores, one merge log, its cuts, labels to the host"), ("set-up", "DerSweep set-up: reference frames, owning windows, upload"),
                    ("score", "DerSweep.score: labels up, xv_diar_confusion, counts down, %d assignments" % (recordings * len(thresholds)))):
        print("diar_tune:   %-90s %s" % (what, show(times[k])))
    # the two ops alone
    ld = (n + 3) // 4 * 4
    buf = torch.zeros(recordings * n * ld, device="cuda")
    for i, x in enumerate(emb.values()):
        xd = torch.from_numpy(x / np.linalg.norm(x, axis=1, keepdims=True)).cuda()
        buf[i * n * ld:(i + 1) * n * ld].view(n, ld)[:, :n] = xd @ xd.T
    nn = np.full(recordings, n, np.int64)
    _, merges, values, n_merges = ops.ahc_cluster(buf, np.arange(recordings, dtype=np.int64) * n * ld, nn, np.full(recordings, ld), targets=np.ones(recordings, np.int64))
    labels, clusters = ops.ahc_cut(merges, values, n_merges, nn, thresholds)
    der = D.DerSweep("cuda:0", reference, subsegs, collar=0.0, overlap="first")
    host_clusters = clusters.cpu().numpy()
    frames = int(der.frames.frames.sum())
    print("diar_tune: ops.ahc_cluster down to one cluster, the %d recordings in one call: %9.1f us" % (recordings, timeit(lambda: ops.ahc_cluster(
        buf, np.arange(recordings, dtype=np.int64) * n * ld, nn, np.full(recordings, ld), targets=np.ones(recordings, np.int64)), 3, 1)))
    print("diar_tune: ops.ahc_cut, %d recordings x %d cuts in one launch (with its four small uploads):        %9.1f us" % (recordings, len(thresholds), timeit(lambda: ops.ahc_cut(merges, values, n_merges, nn, thresholds), 20, 3)))
    print("diar_tune: ops.diar_confusion, %d recordings x %d cuts, %d frames each cut (with its two uploads): %9.1f us; clusters per cut %s" % (
        recordings, len(thresholds), frames, timeit(lambda: ops.diar_confusion(der.frames, labels, host_clusters), 20, 3), " ".join("%d" % c for c in host_clusters.sum(axis=1))), flush=True)


def cmd_vbx(argv):
    """One xv_vbx call over `recordings` recordings of T windows in 128 dimensions started from S speakers (the generator of tests/vbx_ref.py:
    S // 2 true speakers, each split in two), 20 iterations, never stopped: milliseconds per call, medians over five rounds that alternate
    the sizes, and microseconds per iteration of a recording's workgroup.  Beside it, for scale only, the float64 NumPy restatement of the
    same 20 iterations of ONE recording on the CPU."""
    from tf_kaldi_speaker_amd import ops
    from tests import vbx_ref as R
    recordings = int(argv[0]) if argv else 64
    sizes = [tuple(int(v) for v in a.split(",")) for a in argv[1:]] or [(200, 6), (800, 10), (2000, 16)]
    d, iters, (fa, fb, lp) = 128, 20, R.PARAMS[0]
    dev, cpu = {}, {}
    for t, s in sizes:
        cases = [R.make_case(t, d, s, seed) for seed in range(recordings)]
        t0 = time.time()
        R.vbx(cases[0]["x"], cases[0]["phi"], cases[0]["gamma"], cases[0]["pi"], lp, fa, fb, iters, -np.inf, "scaled", np.float64)
        cpu[(t, s)] = (time.time() - t0) * 1e3
        x = torch.from_numpy(np.concatenate([c["x"].ravel() for c in cases])).cuda()
        gamma = torch.from_numpy(np.concatenate([c["gamma"].ravel() for c in cases])).cuda()
        pi = torch.from_numpy(np.concatenate([c["pi"] for c in cases])).cuda()
        dev[(t, s)] = (x, np.arange(recordings, dtype=np.int64) * t * d, np.full(recordings, t, np.int32), torch.from_numpy(cases[0]["phi"].copy()).cuda(),
                       gamma, pi, np.full(recordings, s, np.int32))
    times = {k: [] for k in sizes}
    for _ in range(5):
        for k in sizes:
            x, off, tt, phi, gamma, pi, ss = dev[k]
            times[k].append(timeit(lambda: ops.vbx(x, off, tt, d, phi, gamma, pi, ss, loop_prob=lp, fa=fa, fb=fb, max_iters=iters, epsilon=-np.inf), 2, 1) / 1e3)
    for t, s in sizes:
        med = float(np.median(times[(t, s)]))
        print("vbx: %d recordings x (T, D, S) = (%4d, %d, %2d), %d iterations each: %9.2f ms per call (rounds %s) = %.1f us per iteration of a recording's "
              "workgroup; float64 NumPy restatement, one recording, one CPU: %9.1f ms"
              % (recordings, t, d, s, iters, med, " ".join("%.2f" % v for v in times[(t, s)]), med * 1e3 / iters, cpu[(t, s)]), flush=True)


def cmd_pca_plda(argv):
    """One xv_backend_pca_plda call over b recordings of n windows in D dimensions at a target energy of 0.9 (the four-speaker generator of
    tests/pca_plda_ref.py, one seed per recording): milliseconds per call, medians over five rounds that alternate the shapes.  Beside it the
    host restatement of the same call - tests/pca_plda_ref.py estimate() per recording, NumPy float64 with the BLAS threads the environment
    allows - on this box."""
    from tf_kaldi_speaker_amd import ops
    from tests import pca_plda_ref as P
    shapes = [tuple(int(v) for v in a.split(",")) for a in argv] or [(256, 600, 128), (64, 2048, 200)]
    target = 0.9
    dev, cpu, kept = {}, {}, {}
    for b, n, d in shapes:
        c = P.case(d, n)
        xs = [P.recording(seed, d, n) for seed in range(b)]
        t0 = time.time()
        ref = [P.estimate(x, c["w"], c["b"], c["mu"], target)["p"] for x in xs]
        cpu[(b, n, d)] = (time.time() - t0) * 1e3
        up = lambda a: torch.from_numpy(np.array(a)).cuda()
        dev[(b, n, d)] = (torch.from_numpy(np.concatenate([x.ravel() for x in xs])).cuda(), np.arange(b, dtype=np.int64) * n * d, np.full(b, n, np.int64),
                          up(c["w"]), up(c["b"]), up(c["mu"]))
        got = ops.backend_pca_plda(*dev[(b, n, d)][:3], d, *dev[(b, n, d)][3:], target)
        kept[(b, n, d)] = (got["p"].cpu().numpy(), np.asarray(ref), got["sweeps"].cpu().numpy())
    times = {k: [] for k in shapes}
    for _ in range(5):
        for k in shapes:
            x, off, nn, w, bb, mu = dev[k]
            times[k].append(timeit(lambda: ops.backend_pca_plda(x, off, nn, k[2], w, bb, mu, target), 2, 1) / 1e3)
    for k in shapes:
        p, ref, sweeps = kept[k]
        print("pca_plda: %3d recordings x (n, D) = (%4d, %3d), target 0.9: %9.2f ms per call (rounds %s); kept p %d .. %d (the restatement's for %d of %d), "
              "sweeps %d .. %d and %d .. %d; float64 NumPy restatement, the same recordings one after another: %9.1f ms"
              % (k[0], k[1], k[2], float(np.median(times[k])), " ".join("%.2f" % v for v in times[k]), p.min(), p.max(), int((p == ref).sum()), k[0],
                 sweeps[:, 0].min(), sweeps[:, 0].max(), sweeps[:, 1].min(), sweeps[:, 1].max(), cpu[k]), flush=True)


def cmd_mfcc(argv):
    """Frames per second of xv_mfcc alone and of xv_mfcc + xv_energy_vad on one padded batch (VoxCeleb conf: 16 kHz, 25 / 10 ms, 30 bins, 30
    coefficients); the bytes the kernel has to move (2 S bytes of new samples in, 4 num_ceps bytes out per frame, plus the zeroed padding
    rows) against the 8 TB/s HBM peak show how far from memory-bound it is: LDS traffic and issue rate bound it (csrc/xv_mfcc.hip)."""
    from tf_kaldi_speaker_amd import ops
    n_utts = int(argv[0]) if argv else 256
    sf = 16000
    lens = rs.randint(4 * sf, 20 * sf + 1, n_utts)
    t = np.arange(int(lens.max())) / float(sf)
    tone = 3000.0 * np.sin(2.0 * np.pi * 220.0 * t) + 1500.0 * np.sin(2.0 * np.pi * 1830.0 * t)
    pcm = np.concatenate([np.rint(tone[:n] * (0.02 if i % 3 == 2 else 1.0) + rs.randn(n) * 40.0).astype(np.int16) for i, n in enumerate(lens)])
    offsets = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    cfg = ops.mfcc_config()
    tables = torch.from_numpy(ops.mfcc_tables(cfg)).cuda()
    pcm_d = torch.from_numpy(pcm).cuda()
    frames = np.asarray([ops.mfcc_num_frames(cfg, n) for n in lens])
    t_out = int(frames.max())
    x, rows = ops.mfcc(cfg, tables, pcm_d, offsets, lens, t_out)
    print("%d utterances of %.1f - %.1f s (16 kHz): %.1f M samples, %d frames, padded to [%d, %d, 30]"
          % (n_utts, lens.min() / sf, lens.max() / sf, pcm.size / 1e6, frames.sum(), n_utts, t_out), flush=True)
    us = timeit(lambda: ops.mfcc(cfg, tables, pcm_d, offsets, lens, t_out), 10, 2)
    mb = (2.0 * pcm.size + 4.0 * 30 * n_utts * t_out) / 1e6
    print("  xv_mfcc                 %9.1f us  %.2f M frames/s  (%.0f MB in + out: %.3f TB/s = %.3f of the 8 TB/s peak; includes the offset uploads of ops.py)"
          % (us, frames.sum() / us, mb, mb / us, mb / us / 8.0), flush=True)
    us_vad = timeit(lambda: ops.energy_vad(x, rows), 10, 2)
    print("  xv_energy_vad           %9.1f us  %.2f M frames/s" % (us_vad, frames.sum() / us_vad), flush=True)
    us_both = timeit(lambda: ops.energy_vad(*ops.mfcc(cfg, tables, pcm_d, offsets, lens, t_out)), 10, 2)
    print("  xv_mfcc + xv_energy_vad %9.1f us  %.2f M frames/s = %.0f x real time" % (us_both, frames.sum() / us_both, frames.sum() / us_both * 1e6 / 100.0), flush=True)


def cmd_fbank(argv):
    """xv_fbank (30 bins, the VoxCeleb framing: 16 kHz, 25 / 10 ms, N = 512, d = 30 - the bytes xv_mfcc writes) against xv_mfcc on the batch
    of the mfcc leg, ALTERNATED five times each in one run: per kernel the five timings (each the mean of 10 calls), their median and
    their spread (max - min).  fbank does strictly less work per frame (no DCT, no log-mel slice in LDS), so its median should not lie above
    xv_mfcc's by more than xv_mfcc's own spread; the third column is xv_fbank with energy_out (4 more bytes per frame)."""
    from tf_kaldi_speaker_amd import ops
    n_utts = int(argv[0]) if argv else 256
    sf = 16000
    lens = rs.randint(4 * sf, 20 * sf + 1, n_utts)
    t = np.arange(int(lens.max())) / float(sf)
    tone = 3000.0 * np.sin(2.0 * np.pi * 220.0 * t) + 1500.0 * np.sin(2.0 * np.pi * 1830.0 * t)
    pcm = np.concatenate([np.rint(tone[:n] * (0.02 if i % 3 == 2 else 1.0) + rs.randn(n) * 40.0).astype(np.int16) for i, n in enumerate(lens)])
    offsets = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    mcfg = ops.mfcc_config()
    fcfg = ops.fbank_config(num_mel_bins=30, high_freq=7600.0, snip_edges=0)
    mt, ft = torch.from_numpy(ops.mfcc_tables(mcfg)).cuda(), torch.from_numpy(ops.fbank_tables(fcfg)).cuda()
    pcm_d = torch.from_numpy(pcm).cuda()
    frames = np.asarray([ops.mfcc_num_frames(mcfg, n) for n in lens])
    assert [ops.fbank_num_frames(fcfg, n) for n in lens] == list(frames)
    t_out = int(frames.max())
    print("%d utterances of %.1f - %.1f s (16 kHz): %.1f M samples, %d frames, padded to [%d, %d, 30]"
          % (n_utts, lens.min() / sf, lens.max() / sf, pcm.size / 1e6, frames.sum(), n_utts, t_out), flush=True)
    legs = [("xv_mfcc", lambda: ops.mfcc(mcfg, mt, pcm_d, offsets, lens, t_out)),
            ("xv_fbank", lambda: ops.fbank(fcfg, ft, pcm_d, offsets, lens, t_out, with_energy=False)),
            ("xv_fbank + energy_out", lambda: ops.fbank(fcfg, ft, pcm_d, offsets, lens, t_out))]
    us = {name: [] for name, _ in legs}
    for _ in range(5):
        for name, fn in legs:
            us[name].append(timeit(fn, 10, 2))
    for name, _ in legs:
        v = np.asarray(us[name])
        print("  %-22s %s us  median %8.1f  spread %6.1f  %.2f M frames/s" % (name, " ".join("%8.1f" % x for x in v), np.median(v), v.max() - v.min(),
                                                                              frames.sum() / np.median(v)), flush=True)
    m, f = np.asarray(us["xv_mfcc"]), np.asarray(us["xv_fbank"])
    print("  condition: median(xv_fbank) - median(xv_mfcc) = %+.1f us <= spread(xv_mfcc) = %.1f us: %s"
          % (np.median(f) - np.median(m), m.max() - m.min(), "holds" if np.median(f) - np.median(m) <= m.max() - m.min() else "DOES NOT HOLD"), flush=True)


def cmd_cm_encode(argv):
    """xv_cm_encode on one padded batch of MFCC-like utterances (400 - 2000 frames x 30), both header forms: device events around the bare
    entry point (index arrays uploaded once) and around ops.cm_encode (its checks, two uploads and the output allocation included).  The
    bytes the kernel has to move - 4 rows d read per pass over the piece (quartiles: 1 for the column ranges + 2 ranks x 4 radix passes + 1
    for the codes = 10; uniform: 2) plus rows d written - against the 8 TB/s HBM peak, next to the 0.82 of it a flat streaming kernel
    reaches here; and the host writer dataset.kaldi_io.write_compressed_mat over the same matrices, which is what the kernel replaces."""
    import ctypes as C
    import io
    from tf_kaldi_speaker_amd import _lib, ops
    from tf_kaldi_speaker_amd.dataset import kaldi_io
    n_utts, d = int(argv[0]) if argv else 256, 30
    rows = rs.randint(400, 2001, n_utts)
    t = int(rows.max())
    x_h = np.zeros((n_utts, t, d), np.float32)
    for i, n in enumerate(rows):
        x_h[i, :n] = rs.randn(n, d) * 20.0
        x_h[i, :n, 0] -= 30.0
    x = torch.from_numpy(x_h).cuda()
    values = float(rows.sum()) * d
    print("%d utterances of %d - %d frames x %d: %.2f M frames, %.1f MB of fp32 values" % (n_utts, rows.min(), rows.max(), d, rows.sum() / 1e6, 4 * values / 1e6),
          flush=True)
    p, s = (lambda a: C.c_void_p(a.data_ptr())), (lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream))
    for header, passes in (("quartiles", 10), ("uniform", 2)):
        rows32, offsets, total, code = ops.cm_encode_plan(x.shape, rows, header)
        rows_d, off_d = torch.from_numpy(rows32).cuda(), torch.from_numpy(offsets).cuda()
        out = torch.empty(total, dtype=torch.uint8, device="cuda")
        us = timeit(lambda: _lib.call("xv_cm_encode", s(), p(x), p(rows_d), n_utts, t, d, code, p(off_d), p(out)), 10, 2)
        us_op = timeit(lambda: ops.cm_encode(x, rows, header), 10, 2)
        mb = (4.0 * values * passes + values) / 1e6
        print("  %-9s xv_cm_encode %9.1f us  %.1f M frames/s  (%d passes: %.0f MB read + written = %.3f TB/s = %.3f of the 8 TB/s peak; a flat "
              "streaming kernel: 0.82)   ops.cm_encode %9.1f us" % (header, us, rows.sum() / us, passes, mb, mb / us, mb / us / 8.0, us_op), flush=True)
        t0 = time.perf_counter()
        images = []
        for i, n in enumerate(rows):
            sink = io.BytesIO()
            kaldi_io.write_compressed_mat(sink, x_h[i, :n], header=header)
            images.append(sink.getvalue()[5:])      # behind "\0BCM "
        host_us = (time.perf_counter() - t0) * 1e6
        same = b"".join(images) == out.cpu().numpy().tobytes()
        print("  %-9s write_compressed_mat on the host, one thread: %9.1f us  %.2f M frames/s = %.0f x the kernel's time; the same bytes: %s"
              % (header, host_us, rows.sum() / host_us, host_us / us, same), flush=True)


def cmd_augment(argv):
    """xv_augment on one batch per impulse-response length: every utterance reverberated by the same L taps plus one background noise at 10 dB,
    shift_output and normalize_output on.  Whole calls are timed with device events around ops.augment (table building and the one index
    upload included); the split over the kernel roles comes from torch.profiler's device-side kernel records of one more call (`notrace`
    leaves that out: for a run under rocprofv3 --kernel-trace --stats, which gives the same split from outside).  The FIR's
    rate is priced in taps x samples (one fma each) against the 157.3 TF fp32 vector rate, for the `store` role over n x L and the `energy`
    role over n x (ee - es); the work the kernels skip (taps that meet no sample of a tile) is not subtracted."""
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    from tf_kaldi_speaker_amd import ops
    trace = "notrace" not in argv
    argv = [a for a in argv if a != "notrace"]
    n_utts = int(argv[0]) if argv else 256
    sf = 16000
    lens = rs.randint(4 * sf, 20 * sf + 1, n_utts)
    t = np.arange(int(lens.max())) / float(sf)
    tone = 3000.0 * np.sin(2.0 * np.pi * 220.0 * t) + 1500.0 * np.sin(2.0 * np.pi * 1830.0 * t)
    pcm = np.concatenate([np.rint(tone[:n] * (0.02 if i % 3 == 2 else 1.0) + rs.randn(n) * 40.0).astype(np.int16) for i, n in enumerate(lens)])
    offsets = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    noise = np.rint(rs.randn(5 * sf) * 800.0).astype(np.int16)
    cfg = ops.augment_config()
    pcm_d, noise_d = torch.from_numpy(pcm).cuda(), torch.from_numpy(noise).cuda()
    out = torch.empty(pcm.size, dtype=torch.int16, device="cuda")
    kw = dict(noise=noise_d, noise_off=[0], noise_len=[noise.size], nz_first=np.arange(n_utts + 1), nz_id=np.zeros(n_utts, np.int64),
              nz_snr=np.full(n_utts, 10.0), nz_start=np.zeros(n_utts, np.int64), nz_span=np.full(n_utts, -1), out_pcm=out)
    print("%d utterances of %.1f - %.1f s (16 kHz): %.1f M samples, one background noise each" % (n_utts, lens.min() / sf, lens.max() / sf, pcm.size / 1e6),
          flush=True)
    for L in (0, 4000, 8000, 16000):
        args = dict(kw)
        early = 0
        if L:
            h = np.rint(12000.0 * np.exp(-np.arange(L) / (L / 4.0)) * rs.uniform(-1.0, 1.0, L)).astype(np.int16)
            h[40] = 29000
            es, ee, p = ops.augment_early(h, sf)
            early = ee - es
            args.update(rir=torch.from_numpy(h).cuda(), rir_off=[0], rir_len=[L], rir_early=[(es, ee, p)], utt_rir=np.zeros(n_utts, np.int64))
        call = lambda: ops.augment(cfg, pcm_d, offsets, lens, **args)
        us = timeit(call, 5, 2)
        print("L = %5d taps (early part %3d): whole call %10.1f us = %.0f x real time" % (L, early, us, pcm.size / sf / (us * 1e-6)), flush=True)
        if not trace:
            continue
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            call()
            torch.cuda.synchronize()
        roles = {}
        for ev in prof.events():
            if "aug_" in ev.name and ev.device_type == DeviceType.CUDA:
                name = ev.name.split("(")[0].replace("void ", "")
                roles[name] = roles.get(name, 0.0) + float(getattr(ev, "device_time_total", 0.0) or getattr(ev, "cuda_time_total", 0.0))
        for name, k_us in sorted(roles.items()):
            work = pcm.size * (L if "<false>" in name or "<(bool)0>" in name else early) if "fir" in name else 0
            rate = "  %8.1f G taps x samples / s = %.3f of 157.3 TF" % (work / k_us / 1e3, 2.0 * work / k_us / 1e6 / 157.3) if work else ""
            print("    %-28s %10.1f us%s" % (name, k_us, rate), flush=True)
        if not roles:
            print("    (no kernel records from the profiler: no split over the roles)", flush=True)


def cmd_resample(argv):
    """xv_resample on one ragged batch per conversion.  Device events around the bare entry point (tables and index arrays on the device
    already: the kernel and its memset alone) and around ops.resample (the host checks and the three index uploads included).  The rate is
    priced in fmas (outputs x taps_max, the padding columns included: the kernel runs them) and in the bytes that cross HBM (2 in, 2 out
    per sample)."""
    import ctypes as C
    from tf_kaldi_speaker_amd import _lib, ops
    from tf_kaldi_speaker_amd._host import _p, _s, exclusive_offsets, upload
    from tf_kaldi_speaker_amd.misc.resample import speed_rates
    n_utts = int(argv[0]) if argv else 256
    seconds = rs.uniform(4.0, 20.0, n_utts)
    for label, (fin, fout) in (("16000 -> 8000", (16000, 8000)), ("44100 -> 16000", (44100, 16000)), ("speed 0.9 at 16 kHz", speed_rates("0.9", 16000))):
        cfg = ops.resample_config(fin, fout)
        plan = ops.resample_plan(cfg)
        lens = (seconds * fin).astype(np.int64)
        t = np.arange(int(lens.max())) / float(fin)
        tone = 3000.0 * np.sin(2.0 * np.pi * 220.0 * t) + 1500.0 * np.sin(2.0 * np.pi * 1830.0 * t)
        pcm = np.concatenate([np.rint(tone[:n] + rs.randn(n) * 40.0).astype(np.int16) for n in lens])
        offsets = exclusive_offsets(lens)
        n_out = (lens * plan["out_unit"] + plan["in_unit"] - 1) // plan["in_unit"]
        out_off = exclusive_offsets(n_out)
        pcm_d, tables = torch.from_numpy(pcm).cuda(), torch.from_numpy(ops.resample_tables(cfg)).cuda()
        out = torch.empty(int(n_out.sum()), dtype=torch.int16, device="cuda")
        off_d, n_d, oo_d = upload(offsets, np.int64, out.device), upload(lens, np.int32, out.device), upload(out_off, np.int64, out.device)
        samples, clipped = torch.empty(n_utts, dtype=torch.int32, device="cuda"), torch.empty(n_utts, dtype=torch.int32, device="cuda")
        bare = lambda: _lib.call("xv_resample", _s(), C.byref(cfg), _p(tables), _p(pcm_d), _p(off_d), _p(n_d), n_utts, _p(oo_d), _p(out), _p(None),
                                 _p(samples), _p(clipped))
        whole = lambda: ops.resample(cfg, tables, pcm_d, offsets, lens, out_offsets=out_off, out_pcm=out)
        us_bare, us_whole = timeit(bare, 10, 3), timeit(whole, 10, 3)
        assert np.array_equal(samples.cpu().numpy(), n_out)
        fmas, moved = float(n_out.sum()) * plan["taps_max"], 2.0 * (pcm.size + float(n_out.sum()))
        print("%-20s %d utterances of %.1f - %.1f s: %.1f M samples in, %.1f M out; %d phases x %d taps, tile %d, %d staged samples, %d bytes of LDS"
              % (label, n_utts, seconds.min(), seconds.max(), pcm.size / 1e6, n_out.sum() / 1e6, plan["out_unit"], plan["taps_max"], plan["tile"],
                 plan["span"], plan["lds_bytes"]), flush=True)
        print("    bare entry point %9.1f us = %7.0f x real time, %7.1f G fma / s = %.4f of 157.3 TF, %6.1f GB / s; ops.resample %9.1f us; %d clipped"
              % (us_bare, pcm.size / fin / (us_bare * 1e-6), fmas / us_bare / 1e3, 2.0 * fmas / us_bare / 1e6 / 157.3, moved / us_bare / 1e3, us_whole,
                 int(clipped.sum())), flush=True)


COMMANDS = {"ahc": cmd_ahc, "ahc2": cmd_ahc2, "diar_tune": cmd_diar_tune, "vbx": cmd_vbx, "pca_plda": cmd_pca_plda, "dense": cmd_dense, "resample": cmd_resample, "augment": cmd_augment, "cm_encode": cmd_cm_encode, "mfcc": cmd_mfcc, "fbank": cmd_fbank, "backend": cmd_backend, "plda_cohort": cmd_plda_cohort, "score": cmd_score, "gemm": cmd_gemm, "gemm16": cmd_gemm16, "elementwise": cmd_elementwise, "width": cmd_width, "pitch": cmd_pitch, "pool": cmd_pool, "vlad": cmd_vlad,
            "triplet": cmd_triplet, "ge2e": cmd_ge2e, "segment": cmd_segment, "staged": cmd_staged}

if __name__ == "__main__":
    if len(sys.argv) < 2 or sys.argv[1] not in COMMANDS:
        sys.exit(__doc__)
    COMMANDS[sys.argv[1]](sys.argv[2:])
