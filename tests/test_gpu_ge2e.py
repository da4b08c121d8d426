"""The GE2E training loss of csrc/xv_triplet.hip at op level against the float64 restatement of tests/ge2e_ref.py on the same float32 inputs:
the entries the forward leaves in its workspace (G, n_k, the exclusive norms, c, P), the loss, d w and d b within the derived bounds, d X by
triplet_ref.close_to_f32_eval - both types at the shapes of ge2e_ref.SHAPES (2 x 2 x 4, one speaker, 3 x 2 x 8 at a pitch of 12, 4 x 3 x 512,
13 x 10 x 512: more than 128 rows; 39 x 10 and 64 x 10, softmax only: a thread's second and third column).  x is read at a pitch beyond its
columns with NaN in the padding, the workspace starts as NaN, and d X has NaN behind each row, which must still be there.  Every case is
decision-stable (ge2e_ref: gap >= 64 bounds): the seed is chosen when the case is generated, none is skipped.  Hostile cases, the same bits
from two calls and from a fresh process, the validation loss at w = 20, b = 0, the refusals.  $XV_BOUNDS_OUT names a file that receives the
largest error / bound ratios."""
import atexit
import os
import subprocess
import sys

import numpy as np
import pytest

import ge2e_ref as G
import triplet_ref as R

pytestmark = pytest.mark.gpu

WORST = {}
_CASES = {}
SIZED = [(t, n, m, dim, pad) for n, m, dim, pad, types in G.SHAPES for t in types]      # the contrastive type up to 13 x 10 (ge2e_ref.SHAPES)


def note(name, ratio):
    WORST[name] = max(WORST.get(name, 0.0), float(ratio))


@atexit.register
def _write_ledger():
    path = os.environ.get("XV_BOUNDS_OUT")
    if path and WORST:
        with open(path, "a") as f:
            f.write("# GE2E training loss: largest error / bound over tests/test_gpu_ge2e.py (dx: / the allowance of triplet_ref.close_to_f32_eval)\n")
            for name in sorted(WORST):
                f.write("%-64s %.4f\n" % (name, WORST[name]))


def case(n, m, dim, loss_type):
    """(x, float64 result, float32 NumPy result) of the first decision-stable seed, computed once"""
    key = (n, m, dim, loss_type)
    if key not in _CASES:
        _, x = G.sized_case(n, m, dim, loss_type)
        _CASES[key] = (x, G.ge2e(x, n, m, G.OP_W, G.OP_B, loss_type), G.ge2e(x, n, m, G.OP_W, G.OP_B, loss_type, dt=np.float32))
    return _CASES[key]


@pytest.fixture(scope="module")
def gpu():
    import torch
    from tf_kaldi_speaker_amd import _lib, ops
    return torch, _lib, ops


def run(gpu, loss_type, x, n, m, w, b, pad=4):
    """-> dict(loss, stats, dx, dw, db and the forward's entries g, nk, P, c, ex) through a pitched x with NaN padding, a NaN workspace and a
    NaN-backed dx"""
    torch, _lib, ops = gpu
    rows, d = x.shape
    cfg = ops.ge2e_loss_config(loss_type, n, m)
    xb = torch.full((rows, d + pad), float("nan"), dtype=torch.float32, device="cuda")
    xb[:, :d] = torch.from_numpy(x).to("cuda")
    wt, bt = torch.tensor([w], dtype=torch.float32, device="cuda"), torch.tensor([b], dtype=torch.float32, device="cuda")
    ws = torch.full((int(_lib.load().xv_ge2e_loss_workspace_bytes(n, m, d)) // 4,), float("nan"), dtype=torch.float32, device="cuda")
    loss, stats, ws = ops.ge2e_loss(cfg, xb[:, :d], wt, bt, ws=ws)
    dxb = torch.full((rows, d + 4), float("nan"), dtype=torch.float32, device="cuda")
    _, dw, db = ops.ge2e_loss_backward(cfg, xb[:, :d], wt, bt, ws, out=dxb[:, :d])
    h, f = dxb.cpu().numpy(), ws.cpu().numpy()
    assert np.isnan(h[:, d:]).all(), "xv_ge2e_loss_backward wrote behind a row of dx"
    bp, np_ = (rows + 3) // 4 * 4, (n + 3) // 4 * 4      # the workspace layout of include/xvector_hip.h
    o_n = 3 * rows * bp + 4 * bp + 8
    o_p, o_c, o_e = o_n + np_, o_n + np_ + rows * np_, o_n + np_ + 2 * rows * np_
    return dict(loss=float(loss.cpu()[0]), stats=stats.cpu().numpy(), dx=h[:, :d].copy(), dw=float(dw.cpu()[0]), db=float(db.cpu()[0]),
                g=f[:rows * bp].reshape(rows, bp)[:, :rows], nk=f[o_n:o_n + n], P=f[o_p:o_c].reshape(rows, np_)[:, :n],
                c=f[o_c:o_e].reshape(rows, np_)[:, :n], ex=f[o_e:o_e + rows])


def held(tag, got, ref, bound):
    """every entry within its bound; -> the largest ratio"""
    err = np.abs(R.f64(got) - R.f64(ref))
    ratio = float(np.max(err / (bound + 1e-37)))
    print("    %-22s largest error %.3g, %.3g of its bound" % (tag, float(err.max()), ratio))
    note(tag, ratio)
    assert (err <= bound + 1e-37).all(), "%s: %.3g of the bound" % (tag, ratio)


def compare(tag, got, ref, ev32, rows):
    held(tag + " G", got["g"], R.gram(ref_x(ref), np.float64), R.gram_bound(ref_x(ref)))
    held(tag + " n_k", got["nk"], ref.nk, ref.bnk)
    held(tag + " exclusive norm", got["ex"], ref.ex, ref.bex)
    held(tag + " c", got["c"], ref.c, ref.bc)
    held(tag + " P", got["P"], ref.P, ref.bP)
    held(tag + " loss", got["loss"], ref.loss, ref.bound)
    held(tag + " dw", got["dw"], ref.dw, ref.bound_dw)
    held(tag + " db", got["db"], ref.db, ref.bound_db)
    assert got["stats"][0] == np.float32(got["dw"]) and got["stats"][1] == np.float32(got["db"])
    ok, ratio = R.close_to_f32_eval(got["dx"], ref.dx, ev32.dx, ref.rows_mag, R.gemm_chain(rows))
    print("    dx: %.3g of the allowance, largest |dx| %.3g" % (ratio, np.abs(ref.dx).max()))
    note(tag + " dx", ratio)
    assert ok, "dx: %.3g of the allowance" % ratio


def ref_x(ref):
    return ref.x32


@pytest.mark.parametrize("loss_type,n,m,dim,pad", SIZED, ids=["%s-%dx%dx%d" % c[:4] for c in SIZED])
def test_ge2e_loss_matches_restatement(gpu, loss_type, n, m, dim, pad):
    x, ref, ev32 = case(n, m, dim, loss_type)
    ref.x32 = x
    assert ref.gap >= G.STABLE, "the case is not decision-stable: gap %.3g bounds" % ref.gap
    got = run(gpu, loss_type, x, n, m, G.OP_W, G.OP_B, pad)
    print("%s %dx%dx%d: loss %.9g ref %.9g bound %.3g gap %.3g" % (loss_type, n, m, dim, got["loss"], ref.loss, ref.bound, ref.gap))
    compare(loss_type, got, ref, ev32, n * m)
    if n > 1:
        assert np.abs(ref.dx).max() > 0


@pytest.mark.parametrize("loss_type", G.TYPES)
@pytest.mark.parametrize("name", sorted(G.hostile_cases()))
def test_hostile_cases(gpu, name, loss_type):
    x, w, b = G.hostile_cases()[name]
    ref, ev32 = G.ge2e(x, 4, 2, w, b, loss_type), G.ge2e(x, 4, 2, w, b, loss_type, dt=np.float32)
    ref.x32 = x
    assert ref.gap >= G.STABLE
    got = run(gpu, loss_type, x, 4, 2, w, b)
    assert np.isfinite(got["dx"]).all()
    compare("hostile " + loss_type, got, ref, ev32, 8)
    if name == "w = 0":
        assert got["dw"] == 0 and np.abs(got["dx"]).max() == 0


@pytest.mark.parametrize("loss_type", G.TYPES)
def test_two_calls_give_the_same_bits(gpu, loss_type):
    x, _, _ = case(13, 10, 512, loss_type)
    a, b = run(gpu, loss_type, x, 13, 10, G.OP_W, G.OP_B), run(gpu, loss_type, x, 13, 10, G.OP_W, G.OP_B)
    for k in ("loss", "dw", "db"):
        assert np.float32(a[k]).tobytes() == np.float32(b[k]).tobytes()
    assert a["dx"].tobytes() == b["dx"].tobytes() and a["P"].tobytes() == b["P"].tobytes()


CHILD = """
import sys, numpy as np
sys.path.insert(0, %r)
import torch
import ge2e_ref as G
from tf_kaldi_speaker_amd import ops
_, x = G.sized_case(4, 3, 512, sys.argv[1])
cfg = ops.ge2e_loss_config(sys.argv[1], 4, 3)
xt = torch.from_numpy(x).to("cuda")
w, b = torch.tensor([G.OP_W], device="cuda"), torch.tensor([G.OP_B], device="cuda")
loss, _, ws = ops.ge2e_loss(cfg, xt, w, b)
dx, dw, db = ops.ge2e_loss_backward(cfg, xt, w, b, ws)
print("BITS", np.concatenate([loss.cpu().numpy(), dw.cpu().numpy(), db.cpu().numpy(), dx.cpu().numpy().reshape(-1)]).tobytes().hex())
"""


def test_a_fresh_process_gives_the_same_bits(gpu):
    """the batch alone, here and in a new process: no state of an earlier call, no launch order, enters a sum"""
    here = os.path.dirname(os.path.abspath(__file__))
    x, _, _ = case(4, 3, 512, G.SOFTMAX)
    got = run(gpu, G.SOFTMAX, x, 4, 3, G.OP_W, G.OP_B, pad=0)
    mine = np.concatenate([np.float32([got["loss"], got["dw"], got["db"]]), got["dx"].reshape(-1)]).tobytes().hex()
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.dirname(here), here]))
    out = subprocess.run([sys.executable, "-c", CHILD % here, G.SOFTMAX], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    assert [line.split()[1] for line in out.stdout.splitlines() if line.startswith("BITS")] == [mine]


@pytest.mark.parametrize("n,m,dim", [(4, 3, 512), (13, 10, 512), (2, 2, 4)])
def test_softmax_type_at_w_20_b_0_is_the_validation_loss(gpu, n, m, dim):
    torch, _lib, ops = gpu
    x, _, _ = case(n, m, dim, G.SOFTMAX)
    ref = G.ge2e(x, n, m, 20.0, 0.0, G.SOFTMAX, backward=False)
    got = run(gpu, G.SOFTMAX, x, n, m, 20.0, 0.0)["loss"]
    valid = float(ops.e2e_valid_loss(torch.from_numpy(x).to("cuda"), n, m).cpu()[0])
    print("%dx%dx%d: training %.9g validation %.9g bounds %.3g + %.3g" % (n, m, dim, got, valid, ref.bound, R.e2e_valid_bound(x, n, m)))
    assert abs(got - valid) <= ref.bound + R.e2e_valid_bound(x, n, m)


def test_refusals(gpu):
    torch, _lib, ops = gpu
    x = torch.zeros((8, 8), dtype=torch.float32, device="cuda")
    w, b = torch.ones(1, device="cuda"), torch.zeros(1, device="cuda")
    cfg = ops.ge2e_loss_config("softmax", 4, 2)
    with pytest.raises(ValueError, match="the backward needs the workspace ge2e_loss returned"):
        ops.ge2e_loss_backward(cfg, x, w, b, None)
    small = torch.zeros(16, dtype=torch.float32, device="cuda")
    with pytest.raises(_lib.XvError, match=r"ge2e_loss_backward: the workspace needs \d+ bytes \(xv_ge2e_loss_workspace_bytes\)"):
        ops.ge2e_loss_backward(cfg, x, w, b, small)
    lib = _lib.load()
    assert lib.xv_ge2e_loss_workspace_bytes(8, 1, 8) == 0 and b"at least 2 segments per speaker" in lib.xv_last_error()
    assert lib.xv_ge2e_loss_workspace_bytes(513, 2, 8) == 0 and lib.xv_ge2e_loss_workspace_bytes(4, 2, 6) == 0
    assert b"dimension 6 must be a positive multiple of 4" in lib.xv_last_error()
    bad = ops.ge2e_loss_config("softmax", 4, 2)
    bad.struct_bytes -= 4
    with pytest.raises(_lib.XvError, match="struct_bytes"):
        ops.ge2e_loss(bad, x, w, b)
    bad = ops.ge2e_loss_config("softmax", 4, 2)
    bad.loss_type = 2
    with pytest.raises(_lib.XvError, match="The GE2E only support softmax and contrastive loss"):
        ops.ge2e_loss(bad, x, w, b)
