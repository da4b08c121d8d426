"""The pairwise loss heads of csrc/xv_triplet.hip at op level against the float64 restatement of tests/triplet_ref.py on the same float32
inputs: value within the derived bound, stats exactly, d X by triplet_ref.close_to_f32_eval - every kind and option at 2 (one speaker, no
negatives), 4, 12, 15 (unequal groups, labels not speaker-major) and 130 rows (more than one wave of anchors, more rows than
XV_SEGMENT_MAX_ROWS) by 4, 16 and 512 columns.  x is read at a pitch beyond its columns with NaN in the padding, the workspace starts as NaN,
and d X has NaN behind each row, which must still be there.  Every case is decision-stable (triplet_ref: gap >= 64 bounds): the seed is
chosen when the case is generated, the assertion runs on every case, none is skipped.  Hostile rows (row 1 = row 0, row 2 = -row 0): value
parity, a finite gradient, the stated tie rule.  $XV_BOUNDS_OUT names a file that receives the largest error / bound ratios."""
import atexit
import os

import numpy as np
import pytest

import triplet_ref as R

pytestmark = pytest.mark.gpu

WORST = {}
DIMS = (4, 16, 512)
_CASES = {}


def note(name, ratio):
    WORST[name] = max(WORST.get(name, 0.0), float(ratio))


@atexit.register
def _write_ledger():
    path = os.environ.get("XV_BOUNDS_OUT")
    if path and WORST:
        with open(path, "a") as f:
            f.write("# pairwise loss heads: largest error / bound over tests/test_gpu_triplet.py (dx: / the allowance of triplet_ref.close_to_f32_eval)\n")
            for name in sorted(WORST):
                f.write("%-64s %.4f\n" % (name, WORST[name]))


def case(b, dim, name, kind, opt):
    """(x, labels, float64 result, float32 NumPy result) of the first decision-stable seed, computed once"""
    key = (b, dim, name)
    if key not in _CASES:
        _, (x, lab) = R.stable_case(lambda s: R.sized_case(b, dim, s, kind), lambda c: R.pair_loss(c[0], c[1], kind, backward=False, **opt).gap >= R.STABLE)
        _CASES[key] = (x, lab, R.pair_loss(x, lab, kind, **opt), R.pair_loss(x, lab, kind, dt=np.float32, **opt))
    return _CASES[key]


@pytest.fixture(scope="module")
def gpu():
    import torch
    from tf_kaldi_speaker_amd import _lib, ops
    return torch, _lib, ops


def cfg_of(ops, kind, opt):
    if kind == R.SEMIHARD:
        return ops.pair_loss_config("semihard_triplet_loss", margin=opt["margin"], squared=opt["squared"])
    lt = {v: k for k, v in R.MARGIN_KINDS.items()}[opt["margin_kind"]]
    return ops.pair_loss_config("angular_triplet_loss", margin=opt["margin"], triplet_type=kind, loss_type=lt)


def run(gpu, cfg, x, lab, pad=4):
    """-> (loss, stats [3], dx) through a pitched x with NaN padding, a NaN workspace and a NaN-backed dx"""
    torch, _lib, ops = gpu
    b, d = x.shape
    xb = torch.full((b, d + pad), float("nan"), dtype=torch.float32, device="cuda")
    xb[:, :d] = torch.from_numpy(x).to("cuda")
    y = torch.from_numpy(np.ascontiguousarray(lab, np.int32)).to("cuda")
    ws = torch.full((int(_lib.load().xv_pair_loss_workspace_bytes(b, d)) // 4,), float("nan"), dtype=torch.float32, device="cuda")
    loss, stats, ws = ops.pair_loss(cfg, xb[:, :d], y, ws=ws)
    dxb = torch.full((b, d + 4), float("nan"), dtype=torch.float32, device="cuda")
    ops.pair_loss_backward(cfg, xb[:, :d], y, ws, out=dxb[:, :d])
    h = dxb.cpu().numpy()
    assert np.isnan(h[:, d:]).all(), "xv_pair_loss_backward wrote behind a row of dx"
    return float(loss.cpu()[0]), stats.cpu().numpy()[:3].astype(np.float64), h[:, :d].copy()


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("b", R.SIZES)
@pytest.mark.parametrize("name,kind,opt", R.CONFIGS, ids=[c[0] for c in R.CONFIGS])
def test_pair_loss_matches_restatement(gpu, name, kind, opt, b, dim):
    x, lab, ref, ev32 = case(b, dim, name, kind, opt)
    assert ref.gap >= R.STABLE, "the case is not decision-stable: gap %.3g bounds" % ref.gap
    assert ref.bounded
    loss, stats, dx = run(gpu, cfg_of(gpu[2], kind, opt), x, lab)
    print("%s b=%d d=%d: loss %.9g ref %.9g error %.3g bound %.3g gap %.3g" % (name, b, dim, loss, ref.loss, abs(loss - ref.loss), ref.bound, ref.gap))
    note("loss " + name, abs(loss - ref.loss) / (ref.bound + 1e-37))
    assert abs(loss - ref.loss) <= ref.bound + 1e-37
    assert stats[0] == ref.stats[0] and stats[1] == ref.stats[1] and abs(stats[2] - ref.stats[2]) <= 4 * R.U * ref.stats[2]
    ok, ratio = R.close_to_f32_eval(dx, ref.dx, ev32.dx, ref.rows_mag, R.gemm_chain(b))
    print("    dx: %.3g of the allowance, largest |dx| %.3g" % (ratio, np.abs(ref.dx).max()))
    note("dx " + name, ratio)
    assert ok, "dx: %.3g of the allowance" % ratio
    if ref.loss > 0:
        assert np.abs(ref.dx).max() > 0


@pytest.mark.parametrize("name,kind,opt", R.CONFIGS, ids=[c[0] for c in R.CONFIGS])
def test_more_than_256_rows(gpu, name, kind, opt):
    """390 rows: the second column of a thread (j = tid + 256), seven rounds of the ballot that compacts the positives, two row tiles of the products"""
    x, lab, ref, ev32 = case(390, 16, name, kind, opt)
    assert ref.gap >= R.STABLE and ref.bounded
    loss, stats, dx = run(gpu, cfg_of(gpu[2], kind, opt), x, lab)
    note("loss " + name, abs(loss - ref.loss) / (ref.bound + 1e-37))
    assert abs(loss - ref.loss) <= ref.bound + 1e-37 and stats[0] == ref.stats[0] and stats[1] == ref.stats[1]
    ok, ratio = R.close_to_f32_eval(dx, ref.dx, ev32.dx, ref.rows_mag, R.gemm_chain(390))
    note("dx " + name, ratio)
    assert ok, "dx: %.3g of the allowance" % ratio


@pytest.mark.parametrize("name,kind,opt", R.CONFIGS, ids=[c[0] for c in R.CONFIGS])
def test_two_calls_give_the_same_bits(gpu, name, kind, opt):
    x, lab, _, _ = case(130, 16, name, kind, opt)
    a, b = run(gpu, cfg_of(gpu[2], kind, opt), x, lab), run(gpu, cfg_of(gpu[2], kind, opt), x, lab)
    assert np.float32(a[0]).tobytes() == np.float32(b[0]).tobytes() and a[2].tobytes() == b[2].tobytes()


def hostile(dim=16):
    x, lab = R.embeddings(4, 3, dim, 0, "randn")
    x[1], x[2] = x[0], -x[0]
    return x, lab


@pytest.mark.parametrize("name,kind,opt", R.CONFIGS, ids=[c[0] for c in R.CONFIGS])
def test_hostile_rows(gpu, name, kind, opt):
    """Equal and opposite rows of one speaker: ties in every min / max, |S| = 1, D2 = 0.  No derived bound at the arc margin; the value may be 8 times
    as far from float64 as the float32 NumPy evaluation, and never has to be closer than the derived bound.  The gradient is finite, and
    where the case is tie-free but for the equal rows - whose tie the lowest index takes, here as in the restatement - it matches too."""
    x, lab = hostile()
    xin = R.unit_rows(x) if kind == R.SEMIHARD else x
    ref, ev32 = R.pair_loss(xin, lab, kind, **opt), R.pair_loss(xin, lab, kind, dt=np.float32, **opt)
    loss, stats, dx = run(gpu, cfg_of(gpu[2], kind, opt), xin, lab)
    tol = max(8 * abs(ev32.loss - ref.loss), ref.bound)
    print("%s: loss %.9g ref %.9g error %.3g allowance %.3g" % (name, loss, ref.loss, abs(loss - ref.loss), tol))
    note("hostile loss " + name, abs(loss - ref.loss) / tol)
    assert abs(loss - ref.loss) <= tol
    assert np.isfinite(dx).all()
    assert stats[0] == ref.stats[0]
    if opt.get("margin_kind") != 3:      # the arc margin's slope at |S| = 1 is the clamp's 1e6: finite, not comparable
        ok, ratio = R.close_to_f32_eval(dx, ref.dx, ev32.dx, ref.rows_mag, R.gemm_chain(12))
        note("hostile dx " + name, ratio)
        assert ok, "dx: %.3g of the allowance" % ratio


def test_tie_goes_to_the_lowest_index(gpu):
    """Rows 1 and 2 are equal and the only negatives of row 0 (labels 0, 1, 1; row 3 is row 0's positive): the hardest negative of anchor 0 is a
    tie, and the whole gradient of that term reaches x through row 1 - rows 1 and 2 get different gradients although they hold the same bits."""
    x = R.f32([[1.0, 0.2, 0.0, 0.1], [0.9, 0.35, 0.05, 0.1], [0.9, 0.35, 0.05, 0.1], [0.5, 0.8, 0.3, 0.1]])
    lab = np.asarray([0, 1, 1, 0], np.int32)
    opt = dict(margin=0.1, margin_kind=2)
    ref = R.pair_loss(x, lab, R.HARD, **opt)
    _, _, dx = run(gpu, cfg_of(gpu[2], R.HARD, opt), x, lab)
    assert np.abs(ref.dx[1] - ref.dx[2]).max() > 1e-3
    assert np.abs(dx - ref.dx).max() <= 64 * R.U * np.abs(ref.rows_mag).max()


@pytest.mark.parametrize("n,m,dim", [(1, 2, 4), (2, 2, 4), (4, 3, 16), (5, 2, 8), (3, 4, 512), (13, 10, 16), (1, 5, 8), (6, 1, 8)])
def test_e2e_valid_loss(gpu, n, m, dim):
    torch, _lib, ops = gpu
    x, _ = R.embeddings(n, m, dim, 0, "randn")
    ref, bound = R.e2e_valid_loss(x, n, m), R.e2e_valid_bound(x, n, m)
    xb = torch.full((n * m, dim + 4), float("nan"), dtype=torch.float32, device="cuda")
    xb[:, :dim] = torch.from_numpy(x).to("cuda")
    ws = torch.full((int(_lib.load().xv_pair_loss_workspace_bytes(n * m, dim)) // 4,), float("nan"), dtype=torch.float32, device="cuda")
    got = [float(ops.e2e_valid_loss(xb[:, :dim], n, m, ws=ws).cpu()[0]) for _ in range(2)]
    print("e2e %dx%dx%d: %.9g ref %.9g error %.3g bound %.3g" % (n, m, dim, got[0], ref, abs(got[0] - ref), bound))
    note("e2e_valid_loss", abs(got[0] - ref) / bound)
    assert abs(got[0] - ref) <= bound and got[0] == got[1]


def test_e2e_hostile_rows(gpu):
    torch, _lib, ops = gpu
    x, _ = hostile()
    ref, ev32 = R.e2e_valid_loss(x, 4, 3), R.e2e_valid_loss(x, 4, 3, np.float32)
    got = float(ops.e2e_valid_loss(torch.from_numpy(x).to("cuda"), 4, 3).cpu()[0])
    assert np.isfinite(got) and abs(got - ref) <= max(8 * abs(ev32 - ref), 1e-5 * abs(ref))


def test_limits_are_refused_by_name(gpu):
    torch, _lib, ops = gpu
    cfg = ops.pair_loss_config("semihard_triplet_loss", margin=0.2)
    y = torch.zeros(1025, dtype=torch.int32, device="cuda")
    with pytest.raises(_lib.XvError, match="1025 rows"):
        ops.pair_loss(cfg, torch.zeros((1025, 8), dtype=torch.float32, device="cuda"), y)
    with pytest.raises(_lib.XvError, match="dimension 6 must be a positive multiple of 4"):
        ops.pair_loss(cfg, torch.zeros((8, 6), dtype=torch.float32, device="cuda"), y[:8].contiguous())
    with pytest.raises(_lib.XvError, match="1025 rows"):
        ops.e2e_valid_loss(torch.zeros((1025, 8), dtype=torch.float32, device="cuda"), 205, 5)
    bad = ops.pair_loss_config("angular_triplet_loss", margin=0.2)
    bad.struct_bytes -= 4
    with pytest.raises(_lib.XvError, match="struct_bytes"):
        ops.pair_loss(bad, torch.zeros((8, 8), dtype=torch.float32, device="cuda"), y[:8].contiguous())
    with pytest.raises(NotImplementedError, match="m=3 is not unsupported if asoftmax is selected"):
        ops.pair_loss_config("angular_triplet_loss", margin=3, loss_type="asoftmax")
