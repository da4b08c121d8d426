"""The launch plans of the fp32 GEMMs (csrc/xv_gemm_nt.hip xv_nt_plan, csrc/xv_gemm_tn.hip xv_tn_plan) restated in Python and checked against the library's own
answer (xv_debug_nt_schedule / xv_debug_tn_plan: host arithmetic, no GPU needed) over every layer problem of the S1-S5 shapes and a grid of
ragged ones.  A plan constant changed in the C file without its restatement fails here, naming the shape and the branch; the GPU tests
that run each branch against the float64 oracle (tests/test_gpu_gemm_plans.py) use these restatements to pin the branch of every row."""
import ctypes
import itertools
import os

from tests.test_streamk_schedule import nt_shares

BM = BN = 128
BK = 16
RESIDENT_WGS = 1024            # XV_RESIDENT_WGS: 256 CUs x XV_WGS_PER_CU
NT_SK_WPC = 3                  # XV_NT_SK_WPC
TN_MAX_TILES = 16384           # XV_TN_MAX_TILES (tickets per stream)
TN_AHEAD_MIN = 16              # XV_TN_AHEAD_MIN
TNW_WGS = 512                  # TNW_WGS (xv_gemm_tn160_kernel)
DEBUG_WS = 1 << 32             # the workspace xv_debug_nt_schedule plans with

DP, SK, SHARES, SPLIT = 0, 1, 2, 3
NT_NAMES = {DP: "DP", SK: "SK", SHARES: "SHARES", SPLIT: "SPLIT"}
TN_GENERAL, TN_160 = 0, 1


def cdiv(a, b):
    return -(-a // b)


def nt_plan(M, N, K, stats, co_running, ws_bytes=DEBUG_WS, have_ws=True, forced=0):
    """csrc/xv_gemm_nt.hip xv_nt_plan, restated (forced: XV_NT_SCHED, 1 = dp, 2 = sk).  Returns dict(kind, p_sk, shared_tiles, shares, splits)."""
    tiles, ksteps = cdiv(M, BM) * cdiv(N, BN), cdiv(K, BK)
    total = tiles * ksteps
    p_sk = min(min(256 * NT_SK_WPC, max(1, total // 4)), 8 * tiles)
    t_sk = (total // p_sk) * cdiv(p_sk, 256) + (15 * 16 // BK) * min(NT_SK_WPC, cdiv(p_sk, 256))
    t_dp = cdiv(tiles, 256) * ksteps if tiles <= RESIDENT_WGS else total // 256 + ksteps // 2
    sk = forced == 2 if forced else t_sk + t_sk // 32 < t_dp
    if not forced and co_running and tiles >= 512:
        sk = False
    shares = 0 if (forced or not have_ws or tiles > TN_MAX_TILES or (co_running and ksteps < 100)) else \
        nt_shares(tiles, ksteps, stats, co_running, ws_bytes)
    if shares:
        sk = False
    few = not stats and tiles < 192 and ksteps >= 8 and not forced
    shared_tiles = total % p_sk != 0 or (total // p_sk) % ksteps != 0
    if not few and sk:
        if not shared_tiles or (p_sk * 2 * BM * BN * 4 <= ws_bytes and have_ws and tiles <= TN_MAX_TILES):
            return dict(kind=SK, p_sk=p_sk, shared_tiles=shared_tiles, shares=0, splits=1)
    splits = 1
    if not stats and tiles < RESIDENT_WGS // 2 and ksteps >= 8:
        splits = max(1, min(RESIDENT_WGS // tiles, ksteps // 4))
        np_ = cdiv(N, 4) * 4
        slab_cap = max(8, (8 << 20) // (M * np_ * 4))
        splits = min(splits, slab_cap)
        while splits > 1 and splits * M * np_ * 4 > ws_bytes:
            splits -= 1
    if splits > 1:
        return dict(kind=SPLIT, p_sk=1, shared_tiles=False, shares=0, splits=splits)
    if shares:
        return dict(kind=SHARES, p_sk=1, shared_tiles=False, shares=shares, splits=1)
    return dict(kind=DP, p_sk=1, shared_tiles=False, shares=0, splits=1)


def tn_plan(M, N, R, direct=False):
    """csrc/xv_gemm_tn.hip xv_tn_plan, restated: (kernel, splits, chunk, ahead) - what xv_debug_tn_plan reports."""
    tiles, ksteps = cdiv(M, BM) * cdiv(N, BN), cdiv(R, BK)
    if BM < M <= 160:                                      # xv_gemm_tn160_kernel
        splits = max(1, min(TNW_WGS // cdiv(N, BN), ksteps // 4))
        chunk = cdiv(ksteps, splits) * BK
        return TN_160, cdiv(R, chunk), chunk, 0
    splits = max(1, RESIDENT_WGS // tiles)
    if splits > ksteps // 2:
        splits = max(1, ksteps // 2)
    if direct and ksteps <= 16 and tiles >= 128:
        splits = 1
    if tiles <= 16:
        splits = min(splits, max(1, 256 // tiles))
    chunk = cdiv(ksteps, splits) * BK
    return TN_GENERAL, cdiv(R, chunk), chunk, int(chunk // BK >= TN_AHEAD_MIN)


def wgrad_reduce_zsplit(splits, k, c, o):
    """csrc/xv_gemm_tn.hip xv_launch_wgrad_reduce: the ZSPLIT form (4 groups per output row) or the per-row form"""
    return splits >= 32 and k * c * cdiv(o // 4, 64) < 1024


# ---- the library's answers ---------------------------------------------------------------------------------------------------------
def _lib():
    from tf_kaldi_speaker_amd import _lib as L
    return L.load()


def _per_problem_schedule():
    assert "XV_NT_SCHED" not in os.environ, "XV_NT_SCHED forces the NT schedule: the plan tests need the per-problem choice"


def lib_nt(M, N, K, stats, co_running):
    return _lib().xv_debug_nt_schedule(M, N, K, int(stats), int(co_running))


def lib_tn(M, N, R, direct):
    out = (ctypes.c_int * 4)()
    rc = _lib().xv_debug_tn_plan(M, N, R, int(direct), out)
    assert rc == 0, "xv_debug_tn_plan(%d, %d, %d, %d) failed" % (M, N, R, direct)
    return tuple(out)


# ---- the problems --------------------------------------------------------------------------------------------------------------------
def layer_problems(B, T, layers, feat_pad=32, lout=512, ldl=7352, pool=1500):
    """The GEMM problems of one training step (frame layers as (context, width), xv_engine_fwd.hip / xv_engine_bwd.hip): ("nt", M, N, K, stats, co_running) and
    ("tn", M, N, R, direct)"""
    out = []
    c, t_in = feat_pad, T
    for i, (k, o) in enumerate(layers):
        t_out = t_in - k + 1
        out.append(("nt", B * t_out, o, k * c, True, False))                 # forward + BatchNorm statistics
        if i > 0:
            out.append(("nt", B * t_in, c, k * o, False, True))              # data gradient, beside the weight gradient
        out.append(("tn", k * c, o, B * t_out, False))                       # weight gradient
        c, t_in = o, t_out
    # segment level: tdnn6 (2 x pool -> 512), tdnn7 (512 -> 512), the loss head (512 -> speakers, its weight gradient stored directly)
    for cin, cout in ((2 * pool, 512), (512, lout)):
        out += [("nt", B, cout, cin, True, False), ("nt", B, cin, cout, False, False), ("tn", cin, cout, B, False)]
    out += [("nt", B, ldl, lout, False, False), ("nt", B, lout, ldl, False, False), ("tn", lout, ldl, B, True)]
    return out


REF_LAYERS = ((5, 512), (5, 512), (7, 512), (1, 512), (1, 1500))
S5_LAYERS = ((5, 512), (1, 512), (3, 512), (1, 512), (3, 512), (1, 512), (3, 512), (1, 512), (1, 512), (1, 1500))
WORKLOADS = {"S1": (128, 200, REF_LAYERS), "S2": (128, 400, REF_LAYERS), "S3@200": (64, 200, REF_LAYERS), "S3@300": (64, 300, REF_LAYERS),
             "S3@400": (64, 400, REF_LAYERS), "S4": (128, 200, REF_LAYERS), "S5": (128, 400, S5_LAYERS)}


def _ragged(v):
    return sorted({max(4, v + d) for d in (-16, -12, -4, 0, 4, 12, 16)})


def nt_grid():
    """M, N around 128-row / -column tiles (and the 256-tile rounds), K around 16-column K-steps (K % 4 == 0: the launcher requires it)"""
    Ms = sorted(set(_ragged(128) + _ragged(256) + _ragged(9702) + _ragged(25088) + [1, 37, 285, 5600, 17030, 17550, 32 * 196, 16 * 196]))
    Ns = sorted(set(_ragged(128) + [30, 97, 512, 1499, 1500, 1504, 7352]))
    Ks = sorted(set(_ragged(160) + _ragged(1500) + [4, 8, 12, 68, 512, 2560, 3000, 3584, 7500]))
    return Ms, Ns, Ks


def test_nt_restatement_matches_the_library_on_every_layer_problem():
    _per_problem_schedule()
    bad = []
    n = 0
    for name, (B, T, layers) in WORKLOADS.items():
        for p in layer_problems(B, T, layers):
            if p[0] != "nt":
                continue
            _, M, N, K, stats, co = p
            want, got = nt_plan(M, N, K, stats, co)["kind"], lib_nt(M, N, K, stats, co)
            n += 1
            if want != got:
                bad.append("%s M=%d N=%d K=%d stats=%d co_running=%d: restatement %s, library %s" % (name, M, N, K, stats, co, NT_NAMES[want],
                                                                                                   NT_NAMES.get(got, got)))
    assert n >= 60 and not bad, "\n".join(bad)


def test_nt_restatement_matches_the_library_on_ragged_shapes():
    _per_problem_schedule()
    Ms, Ns, Ks = nt_grid()
    bad, seen = [], set()
    for M, N, K in itertools.product(Ms, Ns, Ks):
        for stats, co in itertools.product((False, True), repeat=2):
            want, got = nt_plan(M, N, K, stats, co)["kind"], lib_nt(M, N, K, stats, co)
            seen.add(got)
            if want != got:
                bad.append("M=%d N=%d K=%d stats=%d co_running=%d: restatement %s, library %s" % (M, N, K, stats, co, NT_NAMES[want], NT_NAMES.get(got, got)))
    assert not bad, "%d disagreements, first: %s" % (len(bad), "\n".join(bad[:20]))
    assert seen == {DP, SK, SHARES, SPLIT}                                   # the grid reaches every branch


def test_tn_restatement_matches_the_library():
    probs = set()
    for B, T, layers in WORKLOADS.values():
        probs |= {(p[1], p[2], p[3]) for p in layer_problems(B, T, layers) if p[0] == "tn"}
    for M in _ragged(128) + _ragged(160) + [140, 160, 161, 256, 512, 2560, 3584]:
        for N in (96, 124, 132, 512, 1500, 7352):
            for R in _ragged(16) + _ragged(256) + [1, 128, 4096, 5823, 25088, 51200]:
                if M % 4 == 0 and N % 4 == 0:
                    probs.add((M, N, R))
    bad, kinds = [], set()
    for (M, N, R), direct in itertools.product(sorted(probs), (False, True)):
        want, got = tn_plan(M, N, R, direct), lib_tn(M, N, R, direct)
        kinds.add((got[0], got[3]))
        if want != got:
            bad.append("M=%d N=%d R=%d direct=%d: restatement %s, library %s" % (M, N, R, direct, want, got))
    assert not bad, "%d disagreements, first: %s" % (len(bad), "\n".join(bad[:20]))
    assert kinds == {(TN_GENERAL, 0), (TN_GENERAL, 1), (TN_160, 0)}


# ---- invariants ----------------------------------------------------------------------------------------------------------------------
def _tn_grid():
    for M in (4, 64, 124, 128, 132, 140, 156, 160, 164, 256, 512, 1500, 2560, 3584):
        for N in (4, 96, 128, 132, 512, 1500, 7352):
            for R in (1, 15, 16, 17, 100, 128, 255, 256, 257, 1000, 4096, 12544, 25088, 51200):
                yield M, N, R


def test_tn_every_split_is_nonempty_and_whole_k_steps():
    for M, N, R in _tn_grid():
        for direct in (False, True):
            kernel, splits, chunk, ahead = tn_plan(M, N, R, direct)
            assert splits * chunk >= R and (splits - 1) * chunk < R, (M, N, R, direct, splits, chunk)
            assert chunk % 16 == 0 and chunk > 0 and splits >= 1
            assert kernel == (TN_160 if 128 < M <= 160 else TN_GENERAL), (M, kernel)      # tn160 exactly for 129 ... 160 rows
            assert not (kernel == TN_160 and ahead)
            if kernel == TN_GENERAL:
                assert ahead == (chunk // 16 >= TN_AHEAD_MIN)
                tiles = cdiv(M, 128) * cdiv(N, 128)
                assert tiles * splits <= max(RESIDENT_WGS, tiles)                        # at most one co-resident round (or one per tile)
            else:
                assert cdiv(N, 128) * splits <= TNW_WGS


def test_tn_unsplit_rule_only_for_direct_short_many_tile_problems():
    for M, N, R in _tn_grid():
        if 128 < M <= 160:
            assert tn_plan(M, N, R, True) == tn_plan(M, N, R, False)
            continue
        tiles, ksteps = cdiv(M, 128) * cdiv(N, 128), cdiv(R, 16)
        plain, direct = tn_plan(M, N, R, False), tn_plan(M, N, R, True)
        if ksteps <= 16 and tiles >= 128:
            assert direct[1] == 1
        else:
            assert direct == plain, (M, N, R)


def test_tn_advice_cases():
    # the loss head's weight gradient (512 x 7352 over 128 chunks), stored directly: one split; not direct it keeps its splits
    assert lib_tn(512, 7352, 128, True)[:2] == (TN_GENERAL, 1)
    assert lib_tn(512, 7352, 128, False)[1] == 4
    # a layer of >= 128 tiles at R <= 256 (small-batch fine-tuning: k 7, c 512, o 1500 -> 3584 x 1500 = 336 tiles) keeps its splits
    for R in (64, 200, 256):
        kernel, splits, chunk, ahead = lib_tn(7 * 512, 1500, R, False)
        assert kernel == TN_GENERAL and splits == min(RESIDENT_WGS // 336, cdiv(R, 16) // 2) and splits > 1, (R, splits)
    # a 16-tile layer (512 x 512 dense): one workgroup per CU, 16 splits, two-ahead staging
    assert lib_tn(512, 512, 25600, False) == (TN_GENERAL, 16, 1600, 1)
    assert lib_tn(512, 512, 128 * 200, True)[1] == 16
    # tdnn1 at S1 (5 taps x 32 padded channels = 160 rows) in the wide kernel: 128 splits planned, 13 K-steps each cover the 1 568 K-steps
    # in 121 - fewer splits than planned
    assert lib_tn(160, 512, 128 * 196, False) == (TN_160, 121, 208, 0)
    assert lib_tn(140, 512, 40 * 146, False)[:2] == (TN_160, 73)


def test_tn_slabs_fit_the_workspaces():
    """xv_affine_wgrad's slabs fit xv_op_workspace_bytes; the engine sizes its slab space at the largest rows of a layer and with
    xv_op_workspace_bytes (xv_engine.hip, workspace_bytes): a smaller batch's plan must fit the same bytes (the split count is not monotone in R)."""
    ws = _lib().xv_op_workspace_bytes
    ws.restype = ctypes.c_size_t
    for M, N, R in _tn_grid():
        for direct in (False, True):
            splits = tn_plan(M, N, R, direct)[1]
            assert splits * M * N * 4 <= ws(R, M, N), (M, N, R, direct)
    for B, T, layers in WORKLOADS.values():
        engine_ws = ws(B * T, 3000, 3000)
        for p in layer_problems(B, T, layers):
            if p[0] != "tn":
                continue
            _, M, N, R_max, direct = p
            cap = max(tn_plan(M, N, R_max, direct)[1] * M * N * 4, engine_ws)
            for R in range(1, R_max + 1, max(1, R_max // 997)):
                assert tn_plan(M, N, R, direct)[1] * M * N * 4 <= cap, (M, N, R, direct)


def test_nt_plans_of_the_production_problems():
    """the branches the S1 / S3 / S5 launches take (what tests/test_gpu_gemm_plans.py must cover)"""
    _per_problem_schedule()
    # S1: tdnn2's data gradient (25088 x 512 x 2560, beside the weight gradient) is one workgroup per tile
    assert nt_plan(25088, 512, 2560, False, True)["kind"] == DP == lib_nt(25088, 512, 2560, False, True)
    # tdnn5's data gradient at 16 chunks (K = 1500, K % 16 = 12) on the even schedule; at 32 chunks shares (5 taps) or DP (dense)
    assert lib_nt(16 * 196, 1500, 1500, False, True) == SK
    assert lib_nt(32 * 200, 1500, 5 * 1500, False, True) == SHARES
    assert lib_nt(32 * 196, 1500, 1500, False, True) == DP


def test_a_changed_plan_constant_is_caught():
    """The restatements are not tautologies: each changed constant moves at least one problem of the grids above to another branch."""
    Ms, Ns, Ks = nt_grid()
    base = {(M, N, K, s, c): nt_plan(M, N, K, s, c)["kind"] for M, N, K in itertools.product(Ms, Ns, Ks) for s, c in ((0, 0), (0, 1), (1, 0))}
    global NT_SK_WPC, TN_AHEAD_MIN
    keep = NT_SK_WPC, TN_AHEAD_MIN
    try:
        NT_SK_WPC = 4
        assert any(nt_plan(*key)["kind"] != v for key, v in base.items())
        NT_SK_WPC = keep[0]
        TN_AHEAD_MIN = 17
        assert any(tn_plan(M, N, R) != lib_tn(M, N, R, False) for M, N, R in _tn_grid())
    finally:
        NT_SK_WPC, TN_AHEAD_MIN = keep
