"""The launch rules of the split-precision (f16x3) GEMMs (csrc/xv_gemm16_nt.hip: nt16_form - generic or context-window kernel, tile height,
taps, chunks, K-steps and the valid halfs of the last one; xv_tn16_splits / tn16_plan - tiles, splits, rows per split, the collapse of
gap-free rows to one segment, steady or per-row stages) restated in Python and checked against the library's own answers
(xv_debug_gemm16_nt_form / xv_debug_gemm16_tn_plan: host arithmetic, no GPU needed) at every boundary of the rules, over a grid and over
the frame-level problems of the shipped configurations.  The GPU rows of tests/test_gpu_gemm16_forms.py use the restatement to pin the
branch each of them runs."""
import ctypes
import json
import os
import re

import pytest

GENERIC, CONV = 0, 1
BK = 32                        # halfs per K-step (NT), reduction rows per stage (TN)
TN_TARGET_WGS = 512            # two resident workgroups per CU
REF_LAYERS = ((5, 512), (5, 512), (7, 512), (1, 512), (1, 1500))      # (context, width) of the reference network's frame layers


def cdiv(a, b):
    return (a + b - 1) // b


def align8(v):
    return cdiv(v, 8) * 8


# ------------------------------------------------------------------ NT
def conv_span(bm, a_rps, a_pitch, taps):
    """x rows a tile of bm output rows reaches behind its first: one extra (pitch - rps) per segment crossing, plus the taps."""
    return (bm - 1) + (a_pitch - a_rps) * ((bm - 1) // a_rps + 1) + (taps - 1)


def conv_applies(K, lda, a_rps, a_pitch, bm):
    if lda % 32 != 0 or K % lda != 0:
        return 0
    taps = K // lda
    if taps < 2 or a_pitch < a_rps:
        return 0
    return taps if conv_span(bm, a_rps, a_pitch, taps) < bm + 32 else 0


def nt_form(M, N, K, lda, a_rps, a_pitch, stats=False, bwd=False, conv_wr=0):
    """nt16_form, restated -> (kernel, tile rows, taps, chunks, tiles_m, tiles_n, K-steps, valid halfs of the last K-step)."""
    kp = align8(K)
    taps, bm = 0, 128
    if not bwd:
        if conv_wr == 4:
            taps = conv_applies(K, lda, a_rps, a_pitch, 256)
            bm = 256 if taps else 128
        if not taps:
            taps = conv_applies(K, lda, a_rps, a_pitch, 128)
    if taps:
        chunks = lda // 32
        return (CONV, bm, taps, chunks, cdiv(M, bm), cdiv(N, 128), taps * chunks, 32)
    nk = cdiv(kp, BK)
    return (GENERIC, 128, 0, 0, cdiv(M, 128), cdiv(N, 128), nk, kp - (nk - 1) * BK)


def _lib():
    from tf_kaldi_speaker_amd import _lib as L
    return L.load()


def lib_nt_form(M, N, K, lda, a_rps, a_pitch, stats=False, bwd=False, conv_wr=0):
    out = (ctypes.c_int * 8)()
    rc = _lib().xv_debug_gemm16_nt_form(M, N, K, lda, a_rps, a_pitch, int(stats), int(bwd), conv_wr, out)
    assert rc == 0, "xv_debug_gemm16_nt_form failed: %s" % _lib().xv_last_error().decode()
    return tuple(out)


def both_nt(M, N, K, lda, a_rps, a_pitch, stats=False, bwd=False, conv_wr=0):
    want, got = nt_form(M, N, K, lda, a_rps, a_pitch, stats, bwd, conv_wr), lib_nt_form(M, N, K, lda, a_rps, a_pitch, stats, bwd, conv_wr)
    assert got == want, "M=%d N=%d K=%d lda=%d rps=%d pitch=%d stats=%d bwd=%d wr=%d: the library says %r, the rule %r" % (
        M, N, K, lda, a_rps, a_pitch, stats, bwd, conv_wr, got, want)
    kernel, bm, taps, chunks, tiles_m, tiles_n, nk, last = want
    # what the kernels rely on: the x rows of a tile inside its (bm + 32)-row A image; whole chunks; the K-steps cover K; a last step of whole 16-byte pieces
    if kernel == CONV:
        assert conv_span(bm, a_rps, a_pitch, taps) < bm + 32 and taps >= 2 and chunks >= 1 and taps * chunks * 32 == K and not bwd
    else:
        assert last % 8 == 0 and 8 <= last <= 32 and (nk - 1) * BK + last == align8(K)
    assert (tiles_m - 1) * bm < M <= tiles_m * bm and (tiles_n - 1) * 128 < N <= tiles_n * 128
    return want


EPILOGUES = ("plain", "statistics", "bn backward")      # EPI 0, 1, 2 of the NT kernels


def nt_form_name(form, stats=False, bwd=False):
    """The name of an NT launch's form in the ledger."""
    kernel = "generic" if form[0] == GENERIC else "conv %d" % form[1]
    return "nt %s, %s" % (kernel, EPILOGUES[2 if bwd else int(bool(stats))])


def nt_forms(conv_wr=0):
    """Every form nt_form can return for a process with that XV_CONV_WR (the context-window kernel has no bn backward epilogue)."""
    conv = "conv %d" % (256 if conv_wr == 4 else 128)
    return {"nt generic, %s" % e for e in EPILOGUES} | {"nt %s, %s" % (conv, e) for e in EPILOGUES[:2]}


def tn_forms():
    return {"tn %s, %s last stage, %s" % (kind, last, splits) for kind in ("collapsed", "steady", "all-ragged") for last in ("ragged", "whole")
            for splits in ("1 split", "splits")}


def forward_problem(segs, t_in, c_ld, k, o):
    """xv_affine_forward_f16x3 -> (M, N, K, lda, a_rps, a_pitch)"""
    t_out = t_in - k + 1
    return (segs * t_out, o, k * c_ld, c_ld, t_out, t_in)


def dgrad_problem(segs, t_out, o_ld, k, c):
    """xv_affine_dgrad_f16x3 on dz planes padded by k - 1 frames on either side of a segment"""
    return (segs * (t_out + k - 1), c, k * o_ld, o_ld, t_out + k - 1, t_out + 2 * (k - 1))


# k -> (the last a_rps that still takes the context-window kernel, the first that falls back), for 128- and 256-row tiles
CONV_BOUNDARY = {128: {2: (5, 4), 3: (9, 8), 5: (19, 18), 7: (32, 31)}, 256: {5: (37, 36), 7: (64, 63)}}


@pytest.mark.parametrize("bm", [128, 256])
def test_conv_boundary_pairs(bm):
    """The pitch of a segment exceeds its rows by k - 1 in the forward (t_in - t_out) and in the data gradient (t_out + 2 (k - 1) - (t_out +
    k - 1)) alike, so both roles share the pairs; at the last admitted a_rps of k = 5 the tile reaches row 159 of the 160-row image."""
    wr = 4 if bm == 256 else 0
    for k, (inside, outside) in CONV_BOUNDARY[bm].items():
        for c_ld in (32, 64, 96):
            for rps, fits in ((inside, True), (outside, False)):
                # a problem the 256-row rule turns away goes to the 128-row rule, which admits these (36 >= 19, 63 >= 32)
                want = (CONV, bm) if fits else ((CONV, 128) if bm == 256 else (GENERIC, 128))
                fwd = forward_problem(14, rps + k - 1, c_ld, k, 136)
                f = both_nt(*fwd, conv_wr=wr)
                assert f[:2] == want, (k, rps, f)
                assert both_nt(*fwd, stats=True, conv_wr=wr) == f
                dg = dgrad_problem(14, rps - k + 1, c_ld, k, 136)
                assert dg[4] == rps and both_nt(*dg, conv_wr=wr)[:2] == want
                assert (conv_span(bm, rps, rps + k - 1, k) < bm + 32) == fits
    assert conv_span(128, 19, 23, 5) == 159 and conv_span(128, 18, 22, 5) == 163
    assert conv_span(256, 37, 41, 5) == 287 and conv_span(256, 64, 70, 7) == 285


def test_conv_needs_whole_chunks_two_taps_and_no_backward_epilogue():
    assert both_nt(*forward_problem(4, 60, 32, 1, 64))[0] == GENERIC               # one tap
    for c_ld in (8, 16, 24, 40, 48):
        assert both_nt(*forward_problem(4, 60, c_ld, 3, 64))[0] == GENERIC          # lda % 32 != 0
    assert both_nt(*forward_problem(4, 60, 64, 3, 64))[:4] == (CONV, 128, 3, 2)
    assert both_nt(*dgrad_problem(4, 57, 64, 5, 64), bwd=True)[0] == GENERIC
    assert both_nt(*dgrad_problem(4, 57, 64, 5, 64))[:4] == (CONV, 128, 5, 2)
    assert both_nt(266, 64, 160, 32, 19, 18)[0] == GENERIC                          # a pitch below the rows of a segment
    for conv_wr in (0, 2):                                                          # 256-row tiles only when forced
        assert both_nt(*forward_problem(14, 41, 32, 5, 64), conv_wr=conv_wr)[1] == 128


@pytest.mark.parametrize("c_ld,k,nk,last", [(8, 1, 1, 8), (16, 1, 1, 16), (24, 1, 1, 24), (40, 1, 2, 8), (8, 3, 1, 24), (16, 3, 2, 16),
                                            (24, 3, 3, 8), (40, 3, 4, 24), (32, 1, 1, 32), (64, 1, 2, 32), (96, 1, 3, 32)])
def test_generic_k_steps_and_tails(c_ld, k, nk, last):
    f = both_nt(*forward_problem(3, 40, c_ld, k, 96))
    assert (f[0], f[6], f[7]) == (GENERIC, nk, last)


def test_nt_restatement_matches_library_over_a_grid():
    for c_ld in (8, 24, 32, 40, 64, 96, 512):
        for taps in range(1, 10):
            for rps in range(1, 301):
                for wr in (0, 4):
                    both_nt(3 * rps + 1, 136, taps * c_ld, c_ld, rps, rps + taps - 1, conv_wr=wr)
                if rps % 7 == 0:
                    both_nt(3 * rps, 8, taps * c_ld, c_ld, rps, rps + taps - 1, bwd=True)
                    both_nt(3 * rps, 1500, taps * c_ld, c_ld, rps, rps + 2 * (taps - 1), stats=True)      # a wider gap than the taps
                    both_nt(3 * rps, 1500, taps * c_ld, c_ld, rps, rps, stats=True, conv_wr=4)            # no gap


def test_nt_hook_refuses_what_the_launcher_refuses():
    L = _lib()
    out = (ctypes.c_int * 8)()
    assert L.xv_debug_gemm16_nt_form(128, 64, 36, 12, 10, 12, 0, 0, 0, out) != 0 and b"gemm16_nt: lda/ldb must be multiples of 8" in L.xv_last_error()
    assert L.xv_debug_gemm16_nt_form(0, 64, 32, 32, 10, 12, 0, 0, 0, out) != 0 and b"gemm16_nt: empty problem" in L.xv_last_error()
    assert L.xv_debug_gemm16_nt_form(128, 64, 32, 32, 0, 12, 0, 0, 0, out) != 0 and b"gemm16_nt: empty problem" in L.xv_last_error()
    assert L.xv_debug_gemm16_nt_form(128, 64, 32, 32, 10, 12, 1, 1, 0, out) != 0 and b"one epilogue at a time" in L.xv_last_error()
    assert L.xv_debug_gemm16_nt_form(128, 64, 32, 32, 10, 12, 0, 0, 3, out) != 0
    assert L.xv_debug_gemm16_nt_form(128, 64, 32, 32, 10, 12, 0, 0, 0, None) != 0
    # a plane that spans 4 GB: (rows + 1) * lda * 2 bytes with rows = segments * pitch - extents only, nothing is allocated
    rows = (1 << 32) // (512 * 2)
    assert L.xv_debug_gemm16_nt_form(rows - 2, 64, 512, 512, rows - 2, rows - 2, 0, 0, 0, out) == 0
    assert L.xv_debug_gemm16_nt_form(rows - 1, 64, 512, 512, rows - 1, rows - 1, 0, 0, 0, out) != 0 and b"gemm16_nt: a plane spans 4 GB" in L.xv_last_error()
    n = (1 << 32) // (4096 * 2)
    assert L.xv_debug_gemm16_nt_form(128, n - 2, 4096, 4096, 128, 128, 0, 0, 0, out) == 0
    assert L.xv_debug_gemm16_nt_form(128, n - 1, 4096, 4096, 128, 128, 0, 0, 0, out) != 0 and b"gemm16_nt: a plane spans 4 GB" in L.xv_last_error()


# ------------------------------------------------------------------ TN
def tn_splits(M, N, R):
    """xv_tn16_splits, restated: 512 / tiles splits, at most half the 32-row stages, at least one; then what the chunk leaves."""
    tiles = cdiv(M, 128) * cdiv(N, 128)
    ksteps = cdiv(R, BK)
    splits = max(1, min(TN_TARGET_WGS // tiles, ksteps // 2))
    return cdiv(R, cdiv(ksteps, splits) * BK)


def tn_plan(M, N, R, rps, a_pitch, b_pitch):
    """tn16_plan, restated -> (tiles, splits, r_chunk, collapsed, steady)"""
    splits = tn_splits(M, N, R)
    r_chunk = cdiv(cdiv(R, BK), splits) * BK
    collapsed = int(a_pitch == rps and b_pitch == rps)
    eff = R if collapsed else rps
    return (cdiv(M, 128) * cdiv(N, 128), splits, r_chunk, collapsed, int(eff >= BK))


def tn_stages(M, N, R, rps, a_pitch, b_pitch):
    """-> dict(tiles, splits, r_chunk, collapsed, steady, rps: what the kernel sees, stages: per split (whole steady stages, per-row stages,
    whether the last stage is ragged - has rows at or beyond the split's end), mid_segment: a split after the first begins inside a segment)"""
    tiles, splits, r_chunk, collapsed, steady = tn_plan(M, N, R, rps, a_pitch, b_pitch)
    eff = R if collapsed else rps
    stages = []
    for s in range(splits):
        rows = min(R, (s + 1) * r_chunk) - s * r_chunk
        nk = cdiv(rows, BK)
        whole = rows // BK if steady else 0
        stages.append((whole, nk - whole, rows % BK != 0))
    return dict(tiles=tiles, splits=splits, r_chunk=r_chunk, collapsed=collapsed, steady=steady, rps=eff, stages=stages,
                mid_segment=any((s * r_chunk) % eff != 0 for s in range(1, splits)))


def tn_form(M, N, R, rps, a_pitch, b_pitch):
    """The name of a TN launch's form in the ledger: how the stages address their rows, whether the last stage is ragged, one split or several."""
    s = tn_stages(M, N, R, rps, a_pitch, b_pitch)
    kind = "collapsed" if s["collapsed"] else ("steady" if s["steady"] else "all-ragged")
    return "tn %s, %s last stage, %s" % (kind, "ragged" if s["stages"][-1][2] else "whole", "1 split" if s["splits"] == 1 else "splits")


def tn_division_misses(rps, lo, hi):
    """The rows r in [lo, hi) at which the per-row stages' r / rps by a float32 product - (int)((float)r * (1.0f / rps)) - misses the segment
    by one and the kernel's +-1 correction has to act.  (Exhaustively: for rps < 32 there is none below r = 10 186 169, where rps = 15 has
    the first; for rps >= 32 the first multiple of rps can be one - 41 - but there only the last, ragged stage of a launch takes the per-row
    form, and it lies inside the last segment.)"""
    import numpy as np
    r = np.arange(lo, hi, dtype=np.int64)
    seg = (r.astype(np.float32) * (np.float32(1) / np.float32(rps))).astype(np.int64)
    return r[seg != r // rps]


def lib_tn_plan(M, N, R, rps, a_pitch, b_pitch):
    out = (ctypes.c_int * 5)()
    rc = _lib().xv_debug_gemm16_tn_plan(M, N, R, rps, a_pitch, b_pitch, out)
    assert rc == 0, "xv_debug_gemm16_tn_plan failed: %s" % _lib().xv_last_error().decode()
    return tuple(out)


def both_tn(M, N, R, rps, a_pitch, b_pitch):
    want, got = tn_plan(M, N, R, rps, a_pitch, b_pitch), lib_tn_plan(M, N, R, rps, a_pitch, b_pitch)
    assert got == want, "M=%d N=%d R=%d rps=%d pitches %d %d: the library plans %r, the rule says %r" % (M, N, R, rps, a_pitch, b_pitch, got, want)
    tiles, splits, r_chunk, collapsed, steady = want
    # what the kernel relies on: whole stages per split, every split non-empty, all of R covered, one co-resident round, a steady stage never wraps twice
    assert r_chunk % BK == 0 and cdiv(R, r_chunk) == splits and (splits - 1) * r_chunk < R
    assert splits * tiles <= max(TN_TARGET_WGS, tiles)
    assert not steady or (R if collapsed else rps) >= BK
    return want


def wgrad_problem(segs, t_in, c_ld, k, o_ld, padded=True):
    """xv_affine_wgrad_f16x3 -> (M, N, R, rps, a_pitch, b_pitch); padded: dz planes with k - 1 zero frames on either side of a segment"""
    t_out = t_in - k + 1
    return (k * c_ld, o_ld, segs * t_out, t_out, t_in, t_out + 2 * (k - 1) if padded else t_out)


def test_tn_split_rule_boundaries():
    # one tile: half the stages, 512 at most
    assert [both_tn(128, 128, r, 57, 61, 65)[1] for r in (1, 31, 32, 63, 64, 65, 127, 128, 129)] == [1, 1, 1, 1, 1, 1, 2, 2, 2]
    assert both_tn(128, 128, 96, 57, 61, 65)[1:3] == (1, 96) and both_tn(128, 128, 97, 57, 61, 65)[1:3] == (2, 64)
    assert both_tn(128, 128, 512 * 64, 57, 61, 65)[1:3] == (512, 64) and both_tn(128, 128, 513 * 64, 57, 61, 65)[1:3] == (342, 96)
    # the cap 512 / tiles: 2 x 2 tiles -> 128, 20 x 12 -> 2, 28 x 12 = 336 -> 1, more than 512 tiles -> 0 clamped to 1
    assert both_tn(160, 136, 1 << 20, 57, 61, 65)[:2] == (4, 128)
    assert both_tn(2560, 1504, 25088, 196, 200, 204)[:2] == (240, 2)
    assert both_tn(3584, 1504, 25088, 194, 200, 206)[:2] == (336, 1)
    assert both_tn(3584, 3584, 25088, 194, 200, 206)[:2] == (784, 1)
    # what the chunk leaves: 5 stages in 2 splits -> chunks of 3 stages, 2 splits; 9 stages, 4 splits -> chunks of 3 -> 3 splits
    assert both_tn(128, 128, 5 * 32, 57, 61, 65)[1:3] == (2, 96) and both_tn(128, 128, 9 * 32, 57, 61, 65)[1:3] == (3, 96)


def test_tn_collapse_and_stage_forms():
    assert both_tn(32, 8, 1000, 1, 1, 1)[3:] == (1, 1)            # gap-free one-frame segments: one segment of R rows, steady
    assert both_tn(32, 8, 20, 1, 1, 1)[3:] == (1, 0)              # ... of fewer than 32 rows: per-row stages
    assert both_tn(32, 8, 1000, 1, 1, 3)[3:] == (0, 0)            # the same rows with a padded dz: not collapsed, all-ragged
    assert both_tn(32, 8, 1000, 1, 3, 1)[3:] == (0, 0)
    for rps, steady in ((3, 0), (7, 0), (31, 0), (32, 1), (33, 1), (57, 1)):
        assert both_tn(160, 136, 40 * rps, rps, rps + 4, rps + 8)[3:] == (0, steady)
    s = tn_stages(160, 136, 40 * 57, 57, 61, 65)
    assert s["splits"] == 36 and s["r_chunk"] == 64 and s["mid_segment"] and s["stages"][0] == (2, 0, False) and s["stages"][-1] == (1, 1, True)
    assert tn_form(160, 136, 40 * 57, 57, 61, 65) == "tn steady, ragged last stage, splits"
    assert tn_form(32, 8, 20, 1, 1, 1) == "tn collapsed, ragged last stage, 1 split"
    assert tn_form(32, 8, 64, 7, 9, 11) == "tn all-ragged, whole last stage, 1 split"


def test_tn_restatement_matches_library_over_a_grid():
    sizes = (8, 128, 136, 160, 512, 1504, 3584)
    rps_of = (1, 3, 7, 31, 32, 33, 57, 196, 300)
    for R in range(1, 5001):
        rps = rps_of[R % len(rps_of)]
        gap = (0, 0) if R % 5 == 0 else (R % 3 * 2, R % 4 * 2)
        for M in sizes:
            for N in sizes:
                both_tn(M, N, R, rps, rps + gap[0], rps + gap[1])
    for R in (1 << 20, (1 << 24) - 1):      # (planes below 4 GB: 208 / 200 x R rows of at most 64 halfs)
        for M in (8, 64):
            both_tn(M, 64, R, 200, 204, 208)


def test_tn_hook_refuses_what_the_launcher_refuses():
    L = _lib()
    out = (ctypes.c_int * 5)()
    assert L.xv_debug_gemm16_tn_plan(36, 8, 100, 10, 10, 10, out) != 0 and b"gemm16_tn: lda/ldb/M/N must be multiples of 8" in L.xv_last_error()
    assert L.xv_debug_gemm16_tn_plan(32, 8, 0, 10, 10, 10, out) != 0 and b"gemm16_tn: bad reduction shape" in L.xv_last_error()
    assert L.xv_debug_gemm16_tn_plan(32, 8, 1 << 24, 10, 10, 10, out) != 0 and b"gemm16_tn: bad reduction shape" in L.xv_last_error()
    assert L.xv_debug_gemm16_tn_plan(32, 8, 100, 0, 10, 10, out) != 0 and b"gemm16_tn: bad reduction shape" in L.xv_last_error()
    assert L.xv_debug_gemm16_tn_plan(32, 8, 100, 10, 10, 10, None) != 0
    segs = (1 << 32) // (3584 * 2 * 200)      # a plane that spans 4 GB: extents only
    assert L.xv_debug_gemm16_tn_plan(3584, 512, segs * 200, 200, 200, 204, out) == 0
    assert L.xv_debug_gemm16_tn_plan(3584, 512, (segs + 1) * 200, 200, 200, 204, out) != 0 and b"gemm16_tn: a plane spans 4 GB" in L.xv_last_error()


# ------------------------------------------------------------------ the shipped configurations
def shipped_shapes():
    """(speakers per batch x segments per speaker, min_segment_len, max_segment_len) of every shipped configuration."""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shipped_nnet_conf.json")) as fh:
        shipped = json.load(fh)
    shapes = set()
    for text in shipped.values():
        v = {k: int(re.search(r'"%s"\s*:\s*(\d+)' % k, text).group(1))
             for k in ("num_speakers_per_batch", "num_segments_per_speaker", "min_segment_len", "max_segment_len")}
        shapes.add((v["num_speakers_per_batch"] * v["num_segments_per_speaker"], v["min_segment_len"], v["max_segment_len"]))
    return sorted(shapes)


def frame_problems(B, T, layers=REF_LAYERS, feat_ld=32):
    """The f16x3 problems of the frame layers of one training step: ("fwd" | "dgrad", NT arguments) and ("wgrad", TN arguments)."""
    out = []
    c_ld, t_in = feat_ld, T
    for i, (k, o) in enumerate(layers):
        t_out, o_ld = t_in - k + 1, align8(o)
        out.append(("fwd", forward_problem(B, t_in, c_ld, k, o)))
        if i > 0:
            out.append(("dgrad", dgrad_problem(B, t_out, o_ld, k, c_ld)))
        out.append(("wgrad", wgrad_problem(B, t_in, c_ld, k, o_ld)))
        c_ld, t_in = o_ld, t_out
    return out


def test_shipped_frame_level_problems():
    shapes = shipped_shapes()
    assert (64, 100, 300) in shapes and (64, 200, 400) in shapes
    seen = set()
    for B, lo, hi in shapes:
        for T in range(max(lo, 16), hi + 1):
            for role, p in frame_problems(B, T):
                if role == "wgrad":
                    tiles, splits, r_chunk, collapsed, steady = both_tn(*p)
                    seen.add(("tn", collapsed, steady))
                else:
                    f = both_nt(*p, stats=role == "fwd")
                    seen.add((role, f[0]))
                    if role == "dgrad":
                        assert both_nt(*p, bwd=True)[0] == GENERIC
                    both_nt(*p, stats=role == "fwd", conv_wr=4)
    # the multi-tap layers take the context-window kernel at every shipped length, the one-tap layers the generic one and the collapsed plan;
    # the one configuration with 30-frame segments leaves tdnn2 / tdnn3 22 and 16 output frames: the all-ragged stages
    assert seen == {("fwd", CONV), ("fwd", GENERIC), ("dgrad", CONV), ("dgrad", GENERIC), ("tn", 0, 0), ("tn", 0, 1), ("tn", 1, 1)}, seen
    assert [both_tn(*p)[3:] for role, p in frame_problems(64, 30) if role == "wgrad"] == [(0, 0), (0, 0), (0, 0), (1, 1), (1, 1)]
    s1 = [both_nt(*p, stats=role == "fwd")[:4] for role, p in frame_problems(128, 200) if role == "fwd"]
    assert s1 == [(CONV, 128, 5, 1), (CONV, 128, 5, 16), (CONV, 128, 7, 16), (GENERIC, 128, 0, 0), (GENERIC, 128, 0, 0)]


def test_ctypes_signatures():
    from tf_kaldi_speaker_amd import _lib as L
    res, args = L.SIGNATURES["xv_debug_gemm16_nt_form"]
    assert res is ctypes.c_int and len(args) == 10
    res, args = L.SIGNATURES["xv_debug_gemm16_tn_plan"]
    assert res is ctypes.c_int and len(args) == 7
