"""The kernel choices of BatchNorm's forward statistics (csrc/xv_bn.hip col_stats_form) and of its backward (csrc/xv_bn_bwd.hip
bn_bwd_plan: reduction form, statistics per chunk, chunk count, apply form) restated in Python and checked against the library's own
answers (xv_debug_col_stats_form / xv_debug_bn_bwd_plan: host arithmetic, no GPU needed) at every boundary of the rules and over a grid.
The GPU rows of tests/test_gpu_bn_pool_forms.py use the restatement to pin the form each of them runs."""
import ctypes
import itertools

import pytest

# --- forward statistics ---
FLOAT4, SCALAR = 4, 1
TILE_M = 128                   # rows per statistics tile (XV_TILE_M)
FIN_CH, FIN_LANES, FIN_BATCH = 8, 32, 8      # bn_finalize_kernel / bn_bwd_finalize_kernel: channels x lanes per block, partials per lane and trip
# --- backward ---
CLOSED, POOLED_PASS, PLAIN_PASS, EXTERNAL = 0, 1, 2, 3
ATT, HS, RELU = 1, 2, 4        # template flags of bn_bwd_reduce_pooled_kernel<RELU, HS, ATT>
DENSE, STRIP, SPLIT = 0, 1, 2
BB_ROWS = BBP_ROWS = 64        # rows per reduction chunk (plain pass / pooled pass)
BAF_ROWS = 32                  # rows per strip of the apply pass
PS_LANES = 64                  # chunk lanes of bn_bwd_pooled_stats_kernel
REDUCE_NAMES = {CLOSED: "closed", POOLED_PASS: "pooled pass", PLAIN_PASS: "plain pass", EXTERNAL: "external partials"}
APPLY_NAMES = {DENSE: "dense", STRIP: "strip", SPLIT: "split"}
BASE = 0x7f0000000000          # an address as the allocator hands them out (256-byte aligned)


def cdiv(a, b):
    return (a + b - 1) // b


def col_stats_form(n, ldz, z=BASE, part=BASE):
    """col_stats_form, restated: one pass over whole float4s when the row length and the pitch are multiples of 4 floats and both the
    tensor and the partials start on a 16-byte boundary; the scalar two-pass form otherwise."""
    return FLOAT4 if (n % 4 == 0 and ldz % 4 == 0 and z % 16 == 0 and part % 16 == 0) else SCALAR


def finalize_trips(partials):
    """Trips of a lane's loop in bn_finalize_kernel (partials = tiles) and bn_bwd_finalize_kernel (partials = chunks)."""
    return cdiv(partials, FIN_LANES * FIN_BATCH)


def pooled_pass_geometry(t):
    """launch_bn_bwd_reduce_pooled: row blocks per chunk and rows per block."""
    nsub = cdiv(t, BBP_ROWS)
    return nsub, cdiv(t, nsub)


def bn_bwd_plan(rows, pooled=False, pool_t=1, pad=0, relu=True, has_slope=False, has_dalpha=False, has_wpos=False, has_weights=False,
                split=False, has_pamax=False, ext_chunks=0):
    """bn_bwd_plan, restated -> (reduce, flags, nstat, chunks, apply)."""
    slope = relu and has_slope
    ext = ext_chunks > 0
    nstat = 4 if (slope and has_dalpha) else 3
    if ext:
        chunks = ext_chunks
    elif pooled:
        chunks = (rows // pool_t) * cdiv(pool_t, BBP_ROWS)
    else:
        chunks = cdiv(rows, BB_ROWS)
    closed = pooled and has_wpos and not slope
    if split:
        closed = closed and has_pamax and not has_weights and not ext
    if closed:
        reduce = CLOSED
    elif ext:
        reduce = EXTERNAL
    elif pooled:
        reduce = POOLED_PASS
    else:
        reduce = PLAIN_PASS
    flags = 0
    if reduce == POOLED_PASS:
        flags = (RELU if relu else 0) | (HS if slope else 0) | (ATT if has_weights else 0)
    if split:
        apply = SPLIT
    elif pad == 0 and (not pooled or pool_t >= BAF_ROWS):
        apply = DENSE
    else:
        apply = STRIP
    return reduce, flags, nstat, chunks, apply


def _lib():
    from tf_kaldi_speaker_amd import _lib as L
    return L.load()


def lib_col_stats_form(n, ldz, z=BASE, part=BASE):
    return _lib().xv_debug_col_stats_form(n, ldz, z, part)


def lib_bn_bwd_plan(rows, pooled=False, pool_t=1, pad=0, relu=True, has_slope=False, has_dalpha=False, has_wpos=False, has_weights=False,
                    split=False, has_pamax=False, ext_chunks=0):
    out = (ctypes.c_int * 5)()
    rc = _lib().xv_debug_bn_bwd_plan(rows, int(pooled), pool_t, pad, int(relu), int(has_slope), int(has_dalpha), int(has_wpos),
                                     int(has_weights), int(split), int(has_pamax), ext_chunks, out)
    assert rc == 0, "xv_debug_bn_bwd_plan failed: %s" % _lib().xv_last_error().decode()
    return tuple(out)


def both(**kw):
    rows = kw.pop("rows")
    want, got = bn_bwd_plan(rows, **kw), lib_bn_bwd_plan(rows, **kw)
    assert got == want, "rows=%d %r: the library plans %r, the rule says %r" % (rows, kw, got, want)
    return want


# ------------------------------------------------------------------ forward statistics
@pytest.mark.parametrize("n,ldz,want", [(4, 4, FLOAT4), (124, 124, FLOAT4), (132, 132, FLOAT4), (132, 136, FLOAT4), (1, 1, SCALAR), (30, 30, SCALAR),
                                        (33, 33, SCALAR), (32, 33, SCALAR), (32, 35, SCALAR), (30, 32, SCALAR), (512, 514, SCALAR)])
def test_col_stats_form_by_shape(n, ldz, want):
    assert col_stats_form(n, ldz) == want
    assert lib_col_stats_form(n, ldz) == want


@pytest.mark.parametrize("off_z,off_part,want", [(0, 0, FLOAT4), (4, 0, SCALAR), (0, 4, SCALAR), (8, 0, SCALAR), (12, 12, SCALAR), (16, 48, FLOAT4)])
def test_col_stats_form_by_alignment(off_z, off_part, want):
    for n in (4, 32, 512):
        assert col_stats_form(n, n, BASE + off_z, BASE + off_part) == want
        assert lib_col_stats_form(n, n, BASE + off_z, BASE + off_part) == want
    # an address above 4 GB keeps its low bits through the call
    assert lib_col_stats_form(32, 32, (1 << 40) + 4, 1 << 40) == SCALAR
    assert lib_col_stats_form(32, 32, (1 << 40) + 16, 1 << 40) == FLOAT4


def test_col_stats_form_matches_library_over_a_grid():
    for n in range(1, 70):
        for extra in range(0, 9):
            for off in (0, 4, 8, 16):
                assert lib_col_stats_form(n, n + extra, BASE + off, BASE) == col_stats_form(n, n + extra, BASE + off, BASE), (n, extra, off)
                assert lib_col_stats_form(n, n + extra, BASE, BASE + off) == col_stats_form(n, n + extra, BASE, BASE + off), (n, extra, off)


def test_finalize_second_trip_boundaries():
    """One trip of a lane's loop covers FIN_LANES * FIN_BATCH = 256 partials: rows <= 32 768 forward, rows <= 16 384 in the plain backward."""
    assert finalize_trips(cdiv(32768, TILE_M)) == 1 and finalize_trips(cdiv(32769, TILE_M)) == 2
    assert finalize_trips(bn_bwd_plan(16384)[3]) == 1 and finalize_trips(bn_bwd_plan(16385)[3]) == 2
    assert lib_bn_bwd_plan(16384)[3] == 256 and lib_bn_bwd_plan(16385)[3] == 257


# ------------------------------------------------------------------ backward
@pytest.mark.parametrize("rows,chunks", [(1, 1), (63, 1), (64, 1), (65, 2), (130, 3), (16384, 256), (16385, 257)])
def test_plain_pass_chunks(rows, chunks):
    for pad in (0, 2, 6):
        assert both(rows=rows, pad=pad) == (PLAIN_PASS, 0, 3, chunks, DENSE if pad == 0 else STRIP)


def test_plain_pass_nstat():
    assert both(rows=130, relu=True, has_slope=True, has_dalpha=True)[2] == 4           # prelu
    assert both(rows=130, relu=True, has_slope=True, has_dalpha=False)[2] == 3          # lrelu
    assert both(rows=130, relu=False, has_slope=True, has_dalpha=True)[2] == 3          # no activation: the context does not apply
    assert both(rows=130, relu=True)[2] == 3


@pytest.mark.parametrize("t,nsub,rows_per", [(1, 1, 1), (31, 1, 31), (63, 1, 63), (64, 1, 64), (65, 2, 33), (128, 2, 64), (129, 3, 43), (186, 3, 62)])
def test_pooled_pass_geometry(t, nsub, rows_per):
    assert pooled_pass_geometry(t) == (nsub, rows_per)
    assert nsub * rows_per >= t > (nsub - 1) * rows_per
    for b in (1, 3):
        assert both(rows=b * t, pooled=True, pool_t=t, relu=True, has_slope=True)[3] == b * nsub


@pytest.mark.parametrize("relu,slope,att,flags", [(False, False, False, 0), (False, False, True, ATT), (True, False, False, RELU),
                                                  (True, False, True, RELU | ATT), (True, True, False, RELU | HS), (True, True, True, RELU | HS | ATT),
                                                  (False, True, False, 0), (False, True, True, ATT)])
def test_pooled_pass_instantiations(relu, slope, att, flags):
    plan = both(rows=3 * 64, pooled=True, pool_t=64, relu=relu, has_slope=slope, has_weights=att)
    assert plan[:2] == (POOLED_PASS, flags)
    # with wpos the closed form replaces the pass exactly when no slope applies
    plan = both(rows=3 * 64, pooled=True, pool_t=64, relu=relu, has_slope=slope, has_weights=att, has_wpos=True)
    assert plan[0] == (POOLED_PASS if (relu and slope) else CLOSED)


def test_closed_form_conditions():
    kw = dict(rows=5 * 37, pooled=True, pool_t=37, has_wpos=True)
    assert both(**kw)[0] == CLOSED
    assert both(has_weights=True, **kw)[0] == CLOSED                                     # fp32: attention weights keep the closed form
    assert both(relu=False, **kw)[0] == CLOSED
    assert both(has_slope=True, **kw)[:2] == (POOLED_PASS, RELU | HS)
    assert both(relu=False, has_slope=True, **kw)[0] == CLOSED
    assert both(rows=5 * 37, pooled=True, pool_t=37)[0] == POOLED_PASS                   # no wpos
    assert both(rows=5 * 37, has_wpos=True)[0] == PLAIN_PASS                             # not pooled
    # split precision: pamax, unit weights and no external partials as well
    assert both(split=True, has_pamax=True, **kw)[0] == CLOSED
    assert both(split=True, **kw)[0] == POOLED_PASS
    assert both(split=True, has_pamax=True, has_weights=True, **kw)[:2] == (POOLED_PASS, RELU | ATT)
    assert both(split=True, has_pamax=True, ext_chunks=2, **kw)[0] == EXTERNAL
    assert both(ext_chunks=2, **kw)[0] == CLOSED                                         # fp32 ignores the partials when the closed form applies
    assert both(rows=300, split=True, ext_chunks=3) == (EXTERNAL, 0, 3, 3, SPLIT)


@pytest.mark.parametrize("t,pad,pooled,want", [(31, 0, True, STRIP), (32, 0, True, DENSE), (33, 0, True, DENSE), (31, 0, False, DENSE),
                                               (1, 0, False, DENSE), (1, 0, True, STRIP), (32, 1, True, STRIP), (33, 2, False, STRIP),
                                               (3, 6, False, STRIP)])
def test_apply_form_boundary(t, pad, pooled, want):
    assert both(rows=3 * t, pooled=pooled, pool_t=t if pooled else 1, pad=pad)[4] == want
    assert both(rows=3 * t, pooled=pooled, pool_t=t if pooled else 1, pad=pad, has_wpos=pooled)[4] == want
    assert both(rows=3 * t, pooled=pooled, pool_t=t if pooled else 1, pad=pad, split=True)[4] == SPLIT


def test_restatement_matches_library_over_a_grid():
    flags = list(itertools.product((False, True), repeat=7))
    for t in (1, 5, 31, 32, 33, 63, 64, 65, 129):
        for b in (1, 3, 64):
            for pad in (0, 2):
                for relu, slope, dalpha, wpos, att, split, pamax in flags:
                    if dalpha and not slope:
                        continue
                    for pooled in (False, True):
                        for ext in ((0, 7) if not (relu and slope) else (0,)):
                            both(rows=b * t, pooled=pooled, pool_t=t if pooled else 1, pad=pad, relu=relu, has_slope=slope, has_dalpha=dalpha,
                                 has_wpos=wpos, has_weights=att, split=split, has_pamax=pamax, ext_chunks=ext)


def test_hooks_refuse_what_the_launch_code_refuses():
    L = _lib()
    out = (ctypes.c_int * 5)()
    assert L.xv_debug_bn_bwd_plan(100, 1, 37, 0, 1, 0, 0, 0, 0, 0, 0, 0, out) != 0 and b"whole chunks" in L.xv_last_error()
    assert L.xv_debug_bn_bwd_plan(128, 0, 1, 0, 1, 1, 0, 0, 0, 1, 0, 1, out) != 0 and b"plain ReLU" in L.xv_last_error()
    assert L.xv_debug_bn_bwd_plan(128, 0, 1, 0, 1, 0, 1, 0, 0, 0, 0, 0, out) != 0 and b"slope" in L.xv_last_error()
