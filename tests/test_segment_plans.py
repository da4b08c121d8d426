"""The launch plan of the segment-level GEMM kernel (csrc/xv_skinny.hip sk_plan: column tiles, splits of K, K per split) and the form of
the attention score kernel (csrc/xv_attention.hip att_score_vec) restated in Python and checked against the library's own answers
(xv_debug_segment_plan / xv_debug_att_score_form: host arithmetic, no GPU needed) at every boundary of the rules, over a grid and over
the segment problems of the shipped configurations.  The GPU rows of tests/test_gpu_segment_forms.py and tests/test_gpu_attention_forms.py
use the restatement to pin the branch each of them runs: splits, stages of a full workgroup, stages of the last split, valid floats of
the last stage."""
import ctypes

import pytest

SK_COLS, SK_ROWS, SK_KS = 32, 128, 32      # columns and rows of a workgroup's tile, k per stage
SK_TARGET_WGS = 256                        # one workgroup per CU
SLAB_BYTES = SK_ROWS * SK_COLS * 4         # one split's partial tile
LARGE_WS = 256 << 20                       # what tf_kaldi_speaker_amd.ops hands every call
VECTOR, SCALAR = 1, 0
BASE = 0x7f0000000000                      # an address as the allocator hands them out (256-byte aligned)


def cdiv(a, b):
    return (a + b - 1) // b


def slab_bytes(n, splits):
    """Workspace that `splits` slabs of every column tile take."""
    return splits * cdiv(n, SK_COLS) * SLAB_BYTES


def segment_plan(m, n, k, ws_bytes=LARGE_WS):
    """sk_plan, restated -> (column tiles, splits, k_chunk): 256 / tiles splits, at most k / 64 (two stages per workgroup at least), at least
    one, no more than ws_bytes holds slabs for; the chunk is k / splits rounded up to whole stages, and the splits are what that chunk leaves."""
    assert 0 < m <= SK_ROWS and n > 0 and k > 0 and k % 4 == 0
    tiles = cdiv(n, SK_COLS)
    splits = SK_TARGET_WGS // tiles
    splits = min(splits, max(1, k // (2 * SK_KS)))
    splits = max(splits, 1)
    while splits > 1 and splits * tiles * SLAB_BYTES > ws_bytes:
        splits -= 1
    k_chunk = cdiv(cdiv(k, splits), SK_KS) * SK_KS
    return tiles, cdiv(k, k_chunk), k_chunk


def segment_stages(m, n, k, ws_bytes=LARGE_WS):
    """-> dict(tiles, splits, k_chunk, stages: K-loop trips of a full workgroup, last_stages: of the last split, last_valid: floats of the
    last split's last stage (a multiple of 4 in 4 ... 32), rotation: (whole three-stage rounds, tail steps) of a full workgroup and of the
    last, slab_sum: (by-four rounds, remainder) of the slab sum, (0, 0) without a split)."""
    tiles, splits, k_chunk = segment_plan(m, n, k, ws_bytes)
    last = k - (splits - 1) * k_chunk
    stages, last_stages = k_chunk // SK_KS if splits > 1 else cdiv(k, SK_KS), cdiv(last, SK_KS)
    return dict(tiles=tiles, splits=splits, k_chunk=k_chunk, stages=stages, last_stages=last_stages, last_valid=last - (last_stages - 1) * SK_KS,
                rotation=(divmod(stages, 3), divmod(last_stages, 3)), slab_sum=divmod(splits, 4) if splits > 1 else (0, 0))


def att_score_form(n, ldz, zk=BASE, query=BASE):
    """att_score_vec, restated: column quads when the row length and the pitch are multiples of 4 floats and both operands start on a
    16-byte boundary; the scalar form otherwise."""
    return VECTOR if (n % 4 == 0 and ldz % 4 == 0 and zk % 16 == 0 and query % 16 == 0) else SCALAR


def _lib():
    from tf_kaldi_speaker_amd import _lib as L
    return L.load()


def lib_segment_plan(m, n, k, ws_bytes=LARGE_WS):
    out = (ctypes.c_int * 3)()
    rc = _lib().xv_debug_segment_plan(m, n, k, ws_bytes, out)
    assert rc == 0, "xv_debug_segment_plan failed: %s" % _lib().xv_last_error().decode()
    return tuple(out)


def lib_att_score_form(n, ldz, zk=BASE, query=BASE):
    return _lib().xv_debug_att_score_form(n, ldz, zk, query)


def both(m, n, k, ws_bytes=LARGE_WS):
    want, got = segment_plan(m, n, k, ws_bytes), lib_segment_plan(m, n, k, ws_bytes)
    assert got == want, "m=%d n=%d k=%d ws=%d: the library plans %r, the rule says %r" % (m, n, k, ws_bytes, got, want)
    tiles, splits, k_chunk = want
    # what the kernel relies on: whole stages per split, every split non-empty, all of k covered, the slabs inside the workspace
    assert k_chunk % SK_KS == 0 and (splits - 1) * k_chunk < k <= splits * k_chunk
    assert splits == 1 or splits * tiles * SLAB_BYTES <= ws_bytes
    assert splits == 1 or k_chunk >= 2 * SK_KS
    return want


# ------------------------------------------------------------------ the split rule
ORIENTATION = [      # (n, k, workspace) -> splits, stages of a full workgroup, stages of the last split, valid floats of the last stage
    ((32, 4, LARGE_WS), (1, 1, 1, 4)),
    ((32, 128, LARGE_WS), (2, 2, 2, 32)), ((32, 192, LARGE_WS), (3, 2, 2, 32)), ((32, 256, LARGE_WS), (4, 2, 2, 32)),
    ((32, 320, LARGE_WS), (5, 2, 2, 32)), ((32, 448, LARGE_WS), (7, 2, 2, 32)), ((32, 512, LARGE_WS), (8, 2, 2, 32)),
    ((32, 576, LARGE_WS), (9, 2, 2, 32)),
    ((64, 452, LARGE_WS), (5, 3, 3, 4)), ((33, 196, LARGE_WS), (3, 3, 1, 4)), ((96, 544, LARGE_WS), (6, 3, 2, 32)),
    ((64, 512, 2 * 2 * SLAB_BYTES), (2, 8, 8, 32)), ((64, 512, 2 * 2 * SLAB_BYTES - 1), (1, 16, 16, 32)), ((64, 512, 0), (1, 16, 16, 32)),
    ((32, 128, 0), (1, 4, 4, 32)), ((32, 160, 0), (1, 5, 5, 32)), ((32, 224, 0), (1, 7, 7, 32)),
]


@pytest.mark.parametrize("shape,want", ORIENTATION)
def test_orientation_table(shape, want):
    n, k, ws = shape
    both(128, n, k, ws)
    s = segment_stages(128, n, k, ws)
    assert (s["splits"], s["stages"], s["last_stages"], s["last_valid"]) == want


@pytest.mark.parametrize("n,tiles", [(1, 1), (31, 1), (32, 1), (33, 2), (63, 2), (64, 2), (65, 3)])
def test_column_tiles_around_32(n, tiles):
    for k in (4, 64, 196, 512):
        assert both(128, n, k)[0] == tiles


def test_tile_count_boundaries_of_the_split_target():
    """256 / tiles: 128 tiles still split in two, 129 no longer; 256 tiles give one split, 257 give 256 / 257 = 0, clamped to one."""
    assert both(128, 4096, 512) == (128, 2, 256)
    assert both(128, 4097, 512) == (129, 1, 512)
    assert both(3, 8192, 512) == (256, 1, 512)
    assert both(3, 8193, 512) == (257, 1, 512)
    assert both(3, 8193, 8) == (257, 1, 32)
    assert both(128, 2048, 4096)[1] == 4 and both(128, 2049, 4096)[1] == 3      # 64 / 65 tiles


@pytest.mark.parametrize("s", range(1, 10))
def test_k_around_multiples_of_64(s):
    """k / 64 caps the splits: one more split at every multiple of 64 (a chunk of 64 = two stages); 4 below it the cap is s - 1."""
    for k, cap in ((64 * s - 4, s - 1), (64 * s, s), (64 * s + 4, s)):
        tiles, splits, k_chunk = both(128, 32, k)
        assert splits <= max(cap, 1)
        if k == 64 * s:
            assert (splits, k_chunk) == (s, 64)


@pytest.mark.parametrize("rem", [0, 4, 28])
def test_partial_last_stage(rem):
    for base in (32, 64, 192, 448):
        for n in (32, 64, 96):
            k = base + rem
            both(128, n, k)
            s = segment_stages(128, n, k)
            assert s["last_valid"] % 4 == 0 and 4 <= s["last_valid"] <= 32
            if s["splits"] == 1:
                assert s["last_valid"] == (rem or 32)


@pytest.mark.parametrize("n,k", [(32, 576), (64, 512), (96, 544), (33, 196), (512, 3000)])
def test_workspace_cap(n, k):
    """The slabs of s splits fit exactly: s splits are planned (when k allows them); one byte less: at most s - 1; nothing: no split."""
    free = both(128, n, k)[1]
    for s in range(1, free + 1):
        fit = slab_bytes(n, s)
        tiles, splits, k_chunk = both(128, n, k, fit)
        assert splits <= s and splits == segment_plan(128, n, k, fit)[1]
        under = both(128, n, k, fit - 1)
        assert under[1] <= max(s - 1, 1)
        if s == free:
            assert splits == free and (under[1] < free or free == 1)
    assert both(128, n, k, 0)[1:] == (1, cdiv(k, 32) * 32)


def test_restatement_matches_library_over_a_grid():
    for n in (1, 31, 32, 33, 64, 96, 100, 512, 1500, 4096, 4097, 7351, 8192, 8193):
        for k in list(range(4, 708, 4)) + [1024, 1500, 3000, 6000, 7352]:
            for ws in (LARGE_WS, 0, slab_bytes(n, 2), slab_bytes(n, 3) - 1, slab_bytes(n, 7)):
                both(128, n, k, ws)
    for m in (1, 2, 64, 127, 128):      # the rows take no part in the rule
        assert both(m, 96, 544) == both(128, 96, 544)


def segment_problems(P, L, N, B):
    """The (m, n, k) the segment chain of a configuration runs: pooling (2 P) -> tdnn6 (512) -> tdnn7 (L) -> logits (N), and the data gradients
    back (k = the speaker count at its 4-float pitch)."""
    n4 = cdiv(N, 4) * 4
    return [(B, 512, 2 * P), (B, L, 512), (B, N, L), (B, L, n4), (B, 512, L), (B, 2 * P, 512)]


def test_shipped_segment_problems():
    for P in (600, 1500, 3000):
        for L in (128, 256, 512):
            for N in (19, 53, 1211, 5994, 7351, 20011):
                for B in (1, 8, 64, 128):
                    for m, n, k in segment_problems(P, L, N, B):
                        both(m, n, k)
                        both(m, n, k, 64 << 20)
                        s = segment_stages(m, n, k)
                        assert s["splits"] * s["tiles"] <= max(SK_TARGET_WGS, s["tiles"])
    # the forward chain of the shipped S1 configuration (P 1500, L 512, 7351 speakers): 16 splits for tdnn6, 8 for tdnn7, 1 for the logits
    assert [segment_stages(*p)["splits"] for p in segment_problems(1500, 512, 7351, 128)[:3]] == [16, 8, 1]


def test_hook_refuses_what_the_launcher_refuses():
    L = _lib()
    out = (ctypes.c_int * 3)()
    assert L.xv_debug_segment_plan(129, 32, 64, 0, out) != 0 and b"segment gemm: bad shape" in L.xv_last_error()
    assert L.xv_debug_segment_plan(0, 32, 64, 0, out) != 0 and b"segment gemm: bad shape" in L.xv_last_error()
    assert L.xv_debug_segment_plan(128, 32, 66, 0, out) != 0 and b"segment gemm: K/lda/ldb must be multiples of 4" in L.xv_last_error()
    assert L.xv_debug_segment_plan(128, 32, 64, 0, None) != 0


def test_ctypes_signatures():
    from tf_kaldi_speaker_amd import _lib as L
    res, args = L.SIGNATURES["xv_debug_segment_plan"]
    assert res is ctypes.c_int and ctypes.sizeof(args[3]) == ctypes.sizeof(ctypes.c_size_t) and len(args) == 5
    res, args = L.SIGNATURES["xv_debug_att_score_form"]
    assert res is ctypes.c_int and [ctypes.sizeof(a) for a in args[2:]] == [ctypes.sizeof(ctypes.c_void_p)] * 2      # uintptr_t: whole addresses


# ------------------------------------------------------------------ the score kernel's form
@pytest.mark.parametrize("n,ldz,want", [(4, 4, VECTOR), (252, 252, VECTOR), (256, 260, VECTOR), (1500, 1500, VECTOR), (2052, 2056, VECTOR),
                                        (1, 1, SCALAR), (63, 63, SCALAR), (65, 65, SCALAR), (1499, 1499, SCALAR), (256, 257, SCALAR),
                                        (1499, 1500, SCALAR), (256, 258, SCALAR)])
def test_att_score_form_by_shape(n, ldz, want):
    assert att_score_form(n, ldz) == want
    assert lib_att_score_form(n, ldz) == want


@pytest.mark.parametrize("off_zk,off_q,want", [(0, 0, VECTOR), (4, 0, SCALAR), (0, 4, SCALAR), (8, 8, SCALAR), (16, 48, VECTOR)])
def test_att_score_form_by_alignment(off_zk, off_q, want):
    for n in (4, 256, 1500):
        assert att_score_form(n, n, BASE + off_zk, BASE + off_q) == want
        assert lib_att_score_form(n, n, BASE + off_zk, BASE + off_q) == want
    assert lib_att_score_form(256, 256, (1 << 40) + 4, 1 << 40) == SCALAR      # an address above 4 GB keeps its low bits through the call
    assert lib_att_score_form(256, 256, (1 << 40) + 16, 1 << 40) == VECTOR


def test_att_score_form_matches_library_over_a_grid():
    for n in range(1, 70):
        for extra in range(0, 9):
            for off in (0, 4, 8, 16):
                assert lib_att_score_form(n, n + extra, BASE + off, BASE) == att_score_form(n, n + extra, BASE + off, BASE), (n, extra, off)
                assert lib_att_score_form(n, n + extra, BASE, BASE + off) == att_score_form(n, n + extra, BASE, BASE + off), (n, extra, off)
