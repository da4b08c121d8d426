"""The update stage on a real MI355X - what xv_engine_apply drives once the gradients exist: the sum of squares behind
clip-by-global-norm, the clip scale (with the 1 / world factor folded in), and the SGD / momentum / Nesterov / Adam kernels -
against the float64 oracle (oracle/xvector_oracle.py: clip_by_global_norm, sgd_update, momentum_update, adam_update, pinned on the CPU
in tests/test_oracle_vs_torch.py).

Engine rows: one or two optimiser steps on a toy topology, compared with the oracle step evaluated on the GPU's ReLU pattern
(tests/test_gpu_engine.py::oracle_step_with_gpu_relu_pattern).  The clip bound of a row is a known fraction of the oracle's global
norm of that very problem, so every row needs the norm before the engine that clips can be created: an unclipped "probe" engine runs
the same forward / loss / backward first (its gradients must equal the clipping engine's bit for bit).

Tolerances
  variables after a step: 2e-5 of the variable's largest entry + what the 1e-4 gradient tolerance admits through the update (_admitted:
      lr * dg for SGD and momentum - the rule of tests/test_gpu_engine.py::compare_step_with_oracle, with the gradient the optimiser
      saw, after grad_scale and clipping - and the oracle's own sensitivity for Adam).  The second of two steps is compared from the
      engine's own state after the first (see _two_steps).
  optimiser state: the momentum accumulator and Adam's m are linear in the applied gradients: 1e-4 of the slot's largest entry (the
      gradient tolerance); Adam's v is quadratic in them: 2e-4.
  sums of squares (xv_sumsq, xv_l2_reg_loss, the engine's clip norm): SUMSQ_FACTOR x the error of a float32 blocked sum of the same
      data against float64, measured on the CPU in the test (sumsq_bound).
  optimiser kernels on identical inputs: rel_fro 1e-6 / rel_max 1e-5, as tests/test_gpu_ops.py::test_optimizers_and_reductions.
"""
from collections import OrderedDict

import numpy as np
import pytest
import torch

from oracle import xvector_oracle as O
from tests.test_gpu_engine import CASES, EXTENDED, ODD_DIMS, RELU_VARIANTS, _make, oracle_step_with_gpu_relu_pattern
from tests.test_gpu_ops import assert_close, dev, host

pytestmark = pytest.mark.gpu

LR = 0.05
GRAD_TOL = 1e-4
SUMSQ_FACTOR = 4.0


@pytest.fixture(scope="module")
def ops():
    from tf_kaldi_speaker_amd import ops as m
    return m


# ---------------------------------------------------------------------------------------------------------------------------------
# the bound for float32 sums of squares
# ---------------------------------------------------------------------------------------------------------------------------------
def blocked_f32_sum(sq32):
    """float32 blocked sum: blocks of 256 summed in float32, then a float32 sum of the block results."""
    pad = (-sq32.size) % 256
    if pad:
        sq32 = np.concatenate([sq32, np.zeros(pad, np.float32)])
    return sq32.reshape(-1, 256).sum(axis=1, dtype=np.float32).sum(dtype=np.float32)


def sumsq_bound(x32, report=None):
    """Relative error a float32 sum of x^2 may show against the float64 sum: SUMSQ_FACTOR x the error of a float32 blocked sum of the
    same data (fused multiply-adds and another evaluation order are legitimate).

    One blocked sum of one data set is a single draw of a rounding error that is zero-mean: it is often far below its own typical
    size, occasionally exactly 0, and 4 x such a draw is not a bound any float32 sum can be held to.  So "the error" is the largest of
    eight such sums of the same data (the block boundaries moved by 0, 32, ..., 224 elements), and never below half a unit in the
    last place of the float32 result - no float32 result can be closer to the float64 sum than that.
    Measured (CPU) on the data of test_sum_of_squares_kernels: 9.0e-8, 5.4e-8, 7.9e-8 for 1 000, 131 073 and 8 388 611 elements, i.e.
    bounds of 3.6e-7, 2.1e-7 and 3.1e-7; 8.6e-8 for 4.6 M gradient-like values."""
    x32 = np.ascontiguousarray(x32, np.float32).reshape(-1)
    sq32 = x32 * x32
    ref = float((x32.astype(np.float64) ** 2).sum())
    errs = []
    for shift in range(0, 256, 32):
        got = float(blocked_f32_sum(np.concatenate([np.zeros(shift, np.float32), sq32])))
        errs.append(abs(got - ref) / ref)
    half_ulp = float(np.spacing(np.float32(ref))) / 2 / ref
    err = max(max(errs), half_ulp)
    if report is not None:
        report["f32_blocked_sum_rel_err"] = err
    return SUMSQ_FACTOR * err


# ---------------------------------------------------------------------------------------------------------------------------------
# engine rows
# ---------------------------------------------------------------------------------------------------------------------------------
OPTIMIZERS = {
    "sgd": dict(optimizer="sgd"),
    "momentum": dict(optimizer="momentum", momentum=0.9),
    "nesterov": dict(optimizer="momentum", momentum=0.9, use_nesterov=True),
    "adam": dict(optimizer="adam"),
}
AMS = dict(loss_func="additive_margin_softmax", margin_m=0.2, last_layer_linear=True)


def _batch(cfg_o, B, T, seed=42):
    rs = np.random.RandomState(seed)
    return rs.randn(B, T, cfg_o.feat_dim).astype(np.float32), rs.randint(0, cfg_o.num_speakers, B).astype(np.int32)


def _backward(eng, x, labels, step):
    eng.forward(x, True)
    eng.loss(labels, step, True)
    eng.backward(-1)


def _slots(eng, cfg_o):
    """The engine's optimiser state as the oracle keeps it: {name: acc} / {name: (m, v)} (slot k of a variable sits at k * n_train + its offset)."""
    S, n = eng.opt_state.cpu().numpy(), eng.n_train
    out = {}
    for name, (shape, off, trainable) in eng.table.items():
        if not trainable or cfg_o.optimizer == "sgd":
            continue
        cnt = int(np.prod(shape))
        if cfg_o.optimizer == "momentum":
            out[name] = S[off:off + cnt].reshape(shape).astype(np.float64)
        else:
            out[name] = (S[off:off + cnt].reshape(shape).astype(np.float64), S[n + off:n + off + cnt].reshape(shape).astype(np.float64))
    return out


def _seed_slots(eng, cfg_o, seed, t):
    """A state as some earlier steps would have left it: random accumulators / first moments, positive second moments, update count t."""
    if cfg_o.optimizer == "sgd":
        return {}
    rs = np.random.RandomState(seed)
    n = eng.n_train
    S = np.zeros(eng.opt_state.numel(), np.float32)
    S[:n] = 0.01 * rs.randn(n)
    if cfg_o.optimizer == "adam":
        S[n:2 * n] = 1e-4 * (0.05 + rs.rand(n))
    eng.opt_state.copy_(torch.from_numpy(S))
    eng.update_count = t
    state = _slots(eng, cfg_o)
    state["__t__"] = t
    return state


def _is_noise_bias(name):
    """A bias in front of a BatchNorm: its gradient is zero in exact arithmetic, rounding noise on both sides (compare_step_with_oracle)."""
    return name.endswith("/bias") and not name.startswith("softmax")


def _admitted(cfg_o, p, g, dg, state, t, lr):
    """What a gradient error of +-dg in every entry admits in the updated parameter: the oracle's own update at g +- dg against the
    one at g, per entry.  lr * dg for SGD, lr * (1 + momentum) * dg with Nesterov - compare_step_with_oracle's rule - and for Adam
    whatever lr_t * m / (sqrt(v) + eps) makes of it: next to nothing where |g| is far above eps, a lot where the clipped gradient and
    the second moment are down at eps."""
    def update(gg):
        if cfg_o.optimizer == "sgd":
            return O.sgd_update(p, gg, lr)
        if cfg_o.optimizer == "momentum":
            return O.momentum_update(p, gg, state if state is not None else np.zeros_like(p), lr, cfg_o.momentum, cfg_o.use_nesterov)[0]
        m, v = state if state is not None else (np.zeros_like(p), np.zeros_like(p))
        return O.adam_update(p, gg, m, v, t, lr)[0]
    base = update(g)
    return np.maximum(np.abs(update(g + dg) - base), np.abs(update(g - dg) - base))


def _compare_update(eng, cfg_o, V, state, newV, new_state, info, lr, var_tol=2e-5, frozen=()):
    """Variables and optimiser state of the engine after apply() against the oracle step V, state -> newV, new_state (tolerances:
    module docstring)."""
    after, slots = eng.get_variables(), _slots(eng, cfg_o)
    t = state.get("__t__", 0) + 1
    for name, v in after.items():
        ref = newV[name]
        if _is_noise_bias(name):
            continue
        diff = np.abs(v - ref)
        slack = np.zeros_like(diff)
        applied = info["applied_grads"].get(name)
        if applied is not None:
            g = applied.reshape(v.shape)
            slack = _admitted(cfg_o, V[name], g, GRAD_TOL * np.abs(g).max(), state.get(name), t, lr)
            if cfg_o.optimizer == "adam":
                # entries whose gradient is rounding noise step by a noise-signed amount on both sides (compare_step_with_oracle)
                keep = np.abs(g) >= 1e-3 * np.abs(g).max()
                diff, slack = diff[keep], slack[keep]
        excess = diff - slack
        assert excess.max() <= var_tol * max(np.abs(ref).max(), 1e-12), (name, excess.max() / max(np.abs(ref).max(), 1e-12))
        if name in frozen or not O.is_trainable(name) or cfg_o.optimizer == "sgd":
            continue
        if cfg_o.optimizer == "momentum":
            pairs = [("acc", slots[name], new_state[name], GRAD_TOL)]
        else:
            pairs = [("m", slots[name][0], new_state[name][0], GRAD_TOL), ("v", slots[name][1], new_state[name][1], 2 * GRAD_TOL)]
        for what, got, want, tol in pairs:
            err = np.abs(got - want.reshape(got.shape)).max() / max(np.abs(want).max(), 1e-30)
            assert err <= tol, (name, what, err)


def _global_norm(G):
    return O.clip_by_global_norm(G, 1e300)[1]


def _check_engine_norm(eng, flat_grads, grad_scale, info, frozen=(), report=None):
    """The engine's clip norm, sqrt(sumsq) * grad_scale, against the oracle's norm function over exactly the oracle's trainable set.

    Two references.  (1) O.clip_by_global_norm in float64 on the gradients the engine itself held (per variable, so nothing between or
    behind the variables is in it, frozen ones zeroed): within the float32 sum-of-squares bound - a slot counted that is no gradient of
    a trainable variable, or a variable left out, is far above it.  (2) The norm of the oracle step's own float64 gradients: the
    engine's gradients agree with those to 1e-4 of each tensor's largest entry only, so that comparison is held to the triangle
    inequality, | ||a|| - ||b|| | <= ||a - b||, plus the same bound."""
    covered = np.zeros(flat_grads.size, bool)
    G = {}
    for name, (shape, off, trainable) in eng.table.items():
        if trainable:
            cnt = int(np.prod(shape))
            covered[off:off + cnt] = True
            G[name] = np.zeros(shape) if name in frozen else flat_grads[off:off + cnt].reshape(shape).astype(np.float64) * grad_scale
    assert set(G) == {k for k in info["grads"]} == {k for k in eng.table if O.is_trainable(k)}
    assert covered.size == eng.n_train and np.all(flat_grads[~covered] == 0), "alignment padding of the gradient buffer is not zero"
    flat = flat_grads.copy()
    for name in frozen:
        shape, off, _ = eng.table[name]
        flat[off:off + int(np.prod(shape))] = 0
    bound = sumsq_bound(flat, report)
    got = float(np.sqrt(np.float64(eng.clip_sumsq()))) * grad_scale
    want = _global_norm(G)
    oracle_norm = info["global_norm"]
    dist = np.sqrt(sum(((G[k] - (0.0 if k in frozen else info["grads"][k].reshape(G[k].shape) * grad_scale)) ** 2).sum() for k in G))
    if report is not None:
        report.update(engine_norm=got, norm_of_engine_grads=want, oracle_norm=oracle_norm, bound=bound, grad_distance=dist)
    print("clip norm: engine %.9g  float64 over the engine's gradients %.9g (rel %.2e, bound %.2e)  oracle step %.9g (rel %.2e)"
          % (got, want, abs(got - want) / want, bound, oracle_norm, abs(got - oracle_norm) / oracle_norm))
    assert abs(got - want) <= bound * want, (got, want, abs(got - want) / want, bound)
    assert abs(got - oracle_norm) <= dist + bound * oracle_norm, (got, oracle_norm, dist)


def _clipped_row(kw, B, T, ratio, dims=None, grad_scale=1.0, seeded_state=False, frozen=(), via_train_step=False):
    """One clipped optimiser step of the engine against the oracle.  ratio: clip bound / the oracle's global norm of this problem."""
    dims = dims or {}
    step = 1234
    probe, cfg_p, V = _make(kw, B, T, **dims)
    x, labels = _batch(cfg_p, B, T)
    _backward(probe, x, labels, step)
    _, _, plain = oracle_step_with_gpu_relu_pattern(probe, V, cfg_p, x.astype(np.float64), labels, LR, step, {}, grad_scale=grad_scale, frozen=frozen)
    norm = _global_norm(plain["applied_grads"])
    g_probe = probe.grads.clone()

    kw_c = dict(kw, clip_gradient=True, clip_gradient_norm=float(np.float32(ratio * norm)))
    eng, cfg_o, V2 = _make(kw_c, B, T, **dims)
    assert all(np.array_equal(V[k], V2[k]) for k in V)
    state = _seed_slots(eng, cfg_o, 7, 4) if seeded_state else {}
    if via_train_step:
        eng.set_update_filter(frozen)
        assert len(eng.frozen_names) == len(frozen)
        eng.train_step(x, labels, LR, step)
    else:
        _backward(eng, x, labels, step)
        assert torch.equal(eng.grads, g_probe), "the same forward / loss / backward on two engines gave different gradients"
        eng.apply(LR, grad_scale)
    newV, new_state, info = oracle_step_with_gpu_relu_pattern(probe, V, cfg_o, x.astype(np.float64), labels, LR, step, state,
                                                              grad_scale=grad_scale, frozen=frozen)
    assert info["global_norm"] == pytest.approx(norm, rel=1e-12)
    assert (ratio < 1) == (info["global_norm"] > cfg_o.clip_gradient_norm)
    _check_engine_norm(eng, g_probe.cpu().numpy(), grad_scale, info, frozen)
    _compare_update(eng, cfg_o, V, state, newV, new_state, info, LR, frozen=frozen)
    after, slots = eng.get_variables(), _slots(eng, cfg_o)
    for name in frozen:                       # outside the var_list: neither the variable nor its slots move, bit for bit
        assert np.array_equal(after[name], V[name].astype(np.float32)), name
        adam = cfg_o.optimizer == "adam"
        for got, was in zip(slots[name] if adam else (slots[name],), state[name] if adam else (state[name],)):
            assert np.abs(was).max() > 0 and np.array_equal(got, was), name
    probe.close()
    eng.close()


@pytest.mark.parametrize("opt", list(OPTIMIZERS))
def test_bound_far_above_the_norm_is_bit_identical_to_no_clipping(opt):
    """clip / max(norm, clip) == 1.0f exactly and g * 1.0f is exact: a bound of 1e9 leaves variables and optimiser state bit-identical to
    the same step with clip_gradient_norm = 0."""
    kw = dict(AMS, **OPTIMIZERS[opt])
    B, T, step = 6, 40, 1234
    res = []
    for clip in (0.0, 1e9):
        eng, cfg_o, _ = _make(dict(kw, clip_gradient=clip > 0, clip_gradient_norm=clip), B, T)
        x, labels = _batch(cfg_o, B, T)
        _seed_slots(eng, cfg_o, 3, 2)
        before = eng.variables.clone()
        _backward(eng, x, labels, step)
        g = eng.grads.clone()
        eng.apply(LR, 1.0)
        torch.cuda.synchronize()
        assert float((eng.variables - before)[:eng.n_train].abs().max()) > 1e-4
        res.append((g, eng.variables.clone(), eng.opt_state.clone(), eng.grads.clone()))
        eng.close()
    (g0, v0, s0, a0), (g1, v1, s1, a1) = res
    assert torch.equal(g0, g1), "the same backward on two engines gave different gradients"
    assert torch.equal(a1, g1), "the clip scale is not exactly 1.0f under a bound far above the norm"
    assert torch.equal(v0, v1) and torch.equal(s0, s1)


@pytest.mark.parametrize("ratio", [0.5, 0.05], ids=["bound0.5", "bound0.05"])
@pytest.mark.parametrize("opt", list(OPTIMIZERS))
def test_scaled_branch_matches_oracle(opt, ratio):
    _clipped_row(dict(AMS, **OPTIMIZERS[opt]), 6, 40, ratio)


VARIABLE_KINDS = {
    "softmax_with_bias": (CASES[0], {}),
    "ring_loss_and_mhe": (CASES[12], {}),
    "prelu": (RELU_VARIANTS[1], {}),
    "self_attention": (CASES[8], {}),
    "extended_tdnn": (EXTENDED[1]["kw"], dict(B=EXTENDED[1]["B"], T=EXTENDED[1]["T"])),
}


@pytest.mark.parametrize("kind", list(VARIABLE_KINDS))
def test_every_kind_of_trainable_variable_is_in_the_norm_and_nothing_else(kind):
    """softmax bias, ring-loss r, PReLU alpha, the attention query and key layers, an extended frame-layer table: the engine's norm runs
    over [0, n_train) of its flat gradient buffer, the oracle's over its trainable set."""
    kw, shape = VARIABLE_KINDS[kind]
    assert {"softmax_with_bias": kw["loss_func"] == "softmax", "ring_loss_and_mhe": "aux_loss_func" in kw, "prelu": kw.get("network_relu_type") == "prelu",
            "self_attention": kw.get("pooling_type") == "self_attention", "extended_tdnn": "frame_layers" in kw}[kind]
    _clipped_row(kw, shape.get("B", 6), shape.get("T", 40), 0.5)


PADDING_ROWS = {
    "last_layer_no_bn": (CASES[4], dict(B=6, T=40)),
    "D23-P600-L256-N101": (ODD_DIMS[0]["kw"], {k: ODD_DIMS[0][k] for k in ("B", "T", "N", "P", "D", "L")}),
    "D40-P3000-N53": (ODD_DIMS[1]["kw"], {k: ODD_DIMS[1][k] for k in ("B", "T", "N", "P", "D", "L")}),
}


@pytest.mark.parametrize("row", list(PADDING_ROWS))
def test_pitch_padding_of_the_gradient_buffer_does_not_count(row):
    """Variables start on 4-float boundaries and the layers pad odd widths inside: whatever of that lies in [0, n_train) must be zero."""
    kw, c = PADDING_ROWS[row]
    assert kw.get("last_layer_no_bn", False) == (row == "last_layer_no_bn")
    dims = {k: c[k] for k in ("N", "P", "D", "L") if k in c}
    _clipped_row(kw, c["B"], c["T"], 0.5, dims=dims)


@pytest.mark.parametrize("opt", ["momentum", "adam"])
def test_frozen_variables_are_outside_the_norm_and_do_not_move(opt):
    """Engine.set_update_filter: train_step zeroes the frozen gradient ranges before apply, so the norm is the unfrozen trainables' (TF's
    restricted var_list, trainer.py:379-410); the frozen variables and their slots - seeded non-zero here - stay as they were."""
    frozen = ("tdnn/tdnn2_conv/kernel", "tdnn/tdnn3_bn/gamma")
    _clipped_row(dict(AMS, **OPTIMIZERS[opt]), 6, 40, 0.5, seeded_state=True, frozen=frozen, via_train_step=True)


def _two_steps(kw, B, T, scales, bound_ratio, check_reg=False):
    """Two consecutive clipped steps on one engine (forward, loss, backward(-1), apply(lr, scale) - the calls train_step makes), each
    against the oracle from the oracle's own previous state.  The bound is bound_ratio x the first step's scaled norm."""
    probe, cfg_p, V = _make(kw, B, T)
    rs = np.random.RandomState(1)
    batches = [(rs.randn(B, T, 30).astype(np.float32), rs.randint(0, cfg_p.num_speakers, B).astype(np.int32)) for _ in range(2)]
    _backward(probe, batches[0][0], batches[0][1], 0)
    _, _, plain = oracle_step_with_gpu_relu_pattern(probe, V, cfg_p, batches[0][0].astype(np.float64), batches[0][1], LR, 0, {}, grad_scale=scales[0])
    bound = float(np.float32(bound_ratio * _global_norm(plain["applied_grads"])))
    probe.close()
    eng, cfg_o, V = _make(dict(kw, clip_gradient=True, clip_gradient_norm=bound), B, T)
    opt = {}
    for it, ((x, labels), gs) in enumerate(zip(batches, scales)):
        _backward(eng, x, labels, it)
        flat = eng.grads.cpu().numpy()
        newV, new_opt, info = oracle_step_with_gpu_relu_pattern(eng, V, cfg_o, x.astype(np.float64), labels, LR, it, opt, grad_scale=gs)
        assert info["global_norm"] > 1.2 * bound, (it, info["global_norm"], bound)       # the scaled branch, both steps
        eng.apply(LR, gs)
        _check_engine_norm(eng, flat, gs, info)
        _compare_update(eng, cfg_o, V, opt, newV, new_opt, info, LR)
        # The next step starts from what the engine holds - variables, slots and update count, all just held to the oracle's: an
        # optimiser step is no contraction (Adam moves an entry whose gradient is rounding noise by up to lr in a noise-given
        # direction), so two trajectories that agree to rounding after one step need not take the same ReLU pattern in the next.
        V = OrderedDict((k, v.astype(np.float64)) for k, v in eng.get_variables().items())
        opt = _slots(eng, cfg_o)
        opt["__t__"] = eng.update_count
        assert eng.update_count == it + 1
        if check_reg:       # the regulariser is evaluated lazily: after an update it must be that of the updated weights
            _, reg = eng.losses()      # (2e-5: compare_step_with_oracle's bound for it on identical weights)
            want, _ = O.regularization(V, cfg_o)
            assert abs(reg - want) <= 2e-5 * abs(want), (it, reg, want)
            assert abs(reg - info["reg_loss"]) > 1e-3 * abs(want), "the update did not move the regulariser: the check above is vacuous"
    eng.close()


@pytest.mark.parametrize("opt", ["momentum", "adam"])
def test_two_consecutive_clipped_steps(opt):
    """The second step's state was built from clipped gradients; the kernel-layout weight copies and the lazily evaluated regulariser
    follow the update (6 rows per segment-level BatchNorm, as the unclipped two-step test)."""
    _two_steps(dict(AMS, **OPTIMIZERS[opt]), 6, 33, (1.0, 1.0), 0.3, check_reg=True)


@pytest.mark.parametrize("opt", ["sgd", "momentum", "adam"])
def test_grad_scale_is_folded_into_the_clip_and_not_applied_twice(opt):
    """apply(lr, 0.5) then apply(lr, 1/8) on one engine (parallel.py passes 1 / world there): the oracle gets the gradients times that
    scale before clipping.  norm = sqrt(sumsq) * grad_scale, and the optimiser sees scale 1 afterwards."""
    _two_steps(dict(AMS, **OPTIMIZERS[opt]), 6, 33, (0.5, 0.125), 0.1)


# ---------------------------------------------------------------------------------------------------------------------------------
# determinism with clipping on
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opt", ["momentum", "adam"])
def test_clipped_step_replayed_from_a_restored_state_is_bit_identical(opt):
    """One engine, the same variables, state and batch: the clipped step replayed from the restored state gives the same sum of squares,
    variables and optimiser state, bit for bit.  n_train is 4.6 M floats here: the sum of squares runs on its full grid."""
    B, T, N, step = 8, 40, 300, 10
    kw = dict(AMS, **OPTIMIZERS[opt])
    probe, cfg_p, _ = _make(kw, B, T, N=N)
    x, labels = _batch(cfg_p, B, T, seed=9)
    _backward(probe, x, labels, step)
    bound = 0.5 * float(probe.grads.double().norm())
    assert probe.n_train > 16 * 131072
    probe.close()
    eng, cfg_o, _ = _make(dict(kw, clip_gradient=True, clip_gradient_norm=bound), B, T, N=N)
    _seed_slots(eng, cfg_o, 5, 3)
    v0, s0 = eng.variables.clone(), eng.opt_state.clone()
    runs = []
    for _ in range(6):
        eng.variables.copy_(v0)
        eng.opt_state.copy_(s0)
        eng.update_count = 3
        eng.lib.xv_engine_invalidate_weights(eng.h)
        _backward(eng, x, labels, step)
        eng.apply(LR, 1.0)
        ss = eng.clip_sumsq()
        runs.append((ss, eng.variables.clone(), eng.opt_state.clone()))
    eng.close()
    assert np.sqrt(runs[0][0]) > 1.9 * bound and not torch.equal(runs[0][1], v0)
    sums = [r[0] for r in runs]
    print("sum of squares of the replays:", ["%.9g" % s for s in sums])
    for i, (ss, v, s) in enumerate(runs[1:], 1):
        assert ss == sums[0], ("sum of squares differs between replays", sums)
        assert torch.equal(v, runs[0][1]) and torch.equal(s, runs[0][2]), "replay %d differs from the first run" % i


# ---------------------------------------------------------------------------------------------------------------------------------
# the kernels themselves
# ---------------------------------------------------------------------------------------------------------------------------------
# grid caps: 8192 x 256 = 2 097 152 elements for the updates, 512 x 256 = 131 072 for the sums of squares
SIZES = [1, 255, 257, 131071, 131072, 131073, 2097151, 2097152, 2097153, 4300003]      # the last: two full trips of the grid plus a tail
KERNELS = ["sgd", "momentum", "nesterov", "adam"]
PAD, SENTINEL = 300, -77.25
# Adam's hyper-parameters cross the C ABI as floats: the oracle gets the same values (0.9f, 0.999f, 1e-8f, in float64 arithmetic), or
# 1 - 0.999f, which is 1.3e-5 away from 0.001, would be charged to the kernel
B1, B2, EPS = float(np.float32(0.9)), float(np.float32(0.999)), float(np.float32(1e-8))


def _padded(a):
    """Device buffer of a.size + PAD floats, sentinels behind the payload; the view of the payload is what the kernel gets."""
    t = torch.full((a.size + PAD,), SENTINEL, dtype=torch.float32, device="cuda:0")
    t[:a.size] = dev(a)
    return t, t[:a.size]


def _run_kernel(ops, kind, p, g, slots, lr, t, scale, momentum=0.9):
    """One update by the kernel on sentinel-padded buffers, and by the float64 oracle on g * scale; returns [(name, got, want)]."""
    bufs = [_padded(a) for a in [p, g] + list(slots)]
    views = [b[1] for b in bufs]
    p64, g64 = p.astype(np.float64), g.astype(np.float64) * scale
    s64 = [s.astype(np.float64) for s in slots]
    if kind == "sgd":
        ops.sgd_update(views[0], views[1], lr, scale)
        want = [O.sgd_update(p64, g64, lr)]
        names = ["p"]
    elif kind in ("momentum", "nesterov"):
        ops.momentum_update(views[0], views[1], views[2], lr, momentum, kind == "nesterov", scale)
        want = list(O.momentum_update(p64, g64, s64[0], lr, momentum, kind == "nesterov"))
        names = ["p", "acc"]
    else:
        ops.adam_update(views[0], views[1], views[2], views[3], lr, t, grad_scale=scale)
        want = list(O.adam_update(p64, g64, s64[0], s64[1], t, lr, B1, B2, EPS))
        names = ["p", "m", "v"]
    torch.cuda.synchronize()
    for full, _ in bufs:
        assert bool((full[p.size:] == SENTINEL).all()), "%s wrote behind count = %d" % (kind, p.size)
    assert np.array_equal(host(views[1]), g.astype(np.float64)), "the gradient buffer was written"
    got = [host(views[0])] + [host(v) for v in views[2:]]
    return list(zip(names, got, want))


def _inputs(kind, n, seed):
    rs = np.random.RandomState(seed)
    p, g = rs.randn(n).astype(np.float32), rs.randn(n).astype(np.float32)
    slots = []
    if kind in ("momentum", "nesterov"):
        slots = [(0.5 * rs.randn(n)).astype(np.float32)]
    elif kind == "adam":
        slots = [(0.1 * rs.randn(n)).astype(np.float32), (1e-3 + 0.5 * rs.rand(n)).astype(np.float32)]
    return p, g, slots


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", KERNELS)
def test_optimizer_kernel_sizes(ops, kind, n):
    """Below, at and above one block, the sumsq grid cap and the update grid cap, and two full trips of the grid-stride loop plus a tail;
    the elements directly behind count stay untouched in every buffer."""
    p, g, slots = _inputs(kind, n, n % 1000 + len(kind))
    res = _run_kernel(ops, kind, p, g, slots, 0.01, 3, 1.0)
    for name, got, want in res:
        assert_close(got, want, 1e-6, 1e-5, "%s %s n=%d" % (kind, name, n))
    assert np.all(res[0][1] != p.astype(np.float64)) or n > 1000      # every parameter moved
    assert np.mean(res[0][1] != p.astype(np.float64)) > 0.99


@pytest.mark.parametrize("scale", [1.0, 0.5, 0.125])
@pytest.mark.parametrize("kind", KERNELS)
def test_optimizer_kernel_grad_scale(ops, kind, scale):
    p, g, slots = _inputs(kind, 100003, 17)
    for name, got, want in _run_kernel(ops, kind, p, g, slots, 0.02, 4, scale):
        assert_close(got, want, 1e-6, 1e-5, "%s %s scale=%g" % (kind, name, scale))
    # and the scale matters: the unscaled update is another one (Adam's step is nearly scale-free, its moments are not)
    if scale != 1.0:
        name, _, want = _run_kernel(ops, kind, p, g, slots, 0.02, 4, scale)[-1]
        _, _, unscaled = _run_kernel(ops, kind, p, g, slots, 0.02, 4, 1.0)[-1]
        assert np.abs(want - unscaled).max() > 1e-3 * np.abs(want).max(), name


@pytest.mark.parametrize("momentum", [0.5, 0.99])
@pytest.mark.parametrize("kind", ["momentum", "nesterov"])
def test_momentum_kernel_non_default_momentum(ops, kind, momentum):
    p, g, slots = _inputs(kind, 100003, 23)
    for name, got, want in _run_kernel(ops, kind, p, g, slots, 0.01, 1, 1.0, momentum=momentum):
        assert_close(got, want, 1e-6, 1e-5, "%s %s momentum=%g" % (kind, name, momentum))


@pytest.mark.parametrize("t", [1, 2, 10, 1000, 100000])
def test_adam_kernel_update_counts_and_gradient_edges(ops, t):
    """The bias correction lr * sqrt(1 - b2^t) / (1 - b1^t) from the first step to where both powers have vanished, on a state the oracle
    ran forward (five steps from zero), with gradients of 0, +-1e-20 and +-1e4 among ordinary ones."""
    n, lr = 100003, 0.001
    rs = np.random.RandomState(t % 97)
    p = rs.randn(n).astype(np.float32)
    edge = np.array([0.0, 1e-20, -1e-20, 1e4, -1e4], np.float32)
    def grad():
        g = rs.randn(n).astype(np.float32)
        g[:50] = np.tile(edge, 10)
        return g
    p64, m64, v64 = p.astype(np.float64), np.zeros(n), np.zeros(n)
    for k in range(1, 6):
        p64, m64, v64 = O.adam_update(p64, grad().astype(np.float64), m64, v64, k, lr, B1, B2, EPS)
    p, m, v = p64.astype(np.float32), m64.astype(np.float32), v64.astype(np.float32)
    assert np.abs(m).max() > 0 and v[3] > 1e4
    g = grad()
    g[50:100] = np.tile(edge, 10)[::-1]                      # and every edge value on a state that an ordinary gradient built
    res = _run_kernel(ops, "adam", p, g, [m, v], lr, t, 1.0)
    for name, got, want in res:
        assert np.all(np.isfinite(got)), name
        assert_close(got, want, 1e-6, 1e-5, "adam %s t=%d" % (name, t))
    # the +-1e4 gradients set the scale of m and v above: the ordinary entries on their own
    for name, got, want in res[1:]:
        assert_close(got[100:], want[100:], 1e-6, 1e-5, "adam %s t=%d, ordinary entries" % (name, t))
    # and the steps themselves, which are ~1e-3 of the parameters: 1e-5 of the largest step plus the rounding of the stored
    # parameter (half a unit in the last place, <= 2^-24 of its size) - this is what sees a wrong bias correction
    _, got, want = res[0]
    step_ref = want - p.astype(np.float64)
    step_err = np.abs((got - p.astype(np.float64)) - step_ref).max()
    assert step_err <= 1e-5 * np.abs(step_ref).max() + 2.0 ** -24 * np.abs(want).max(), (t, step_err, np.abs(step_ref).max())


def _f32_recurrence(kind, p, gs, slots, lr, momentum=0.9):
    """The kernels' recurrences evaluated by NumPy in float32 (one rounding per operation, no fused multiply-add)."""
    f = np.float32
    p = p.copy()
    s = [a.copy() for a in slots]
    for t, g in enumerate(gs, 1):
        if kind == "sgd":
            p = p - f(lr) * g
        elif kind in ("momentum", "nesterov"):
            s[0] = f(momentum) * s[0] + g
            p = p - f(lr) * (g + f(momentum) * s[0]) if kind == "nesterov" else p - f(lr) * s[0]
        else:
            lr_t = f(lr * np.sqrt(1.0 - B2 ** t) / (1.0 - B1 ** t))
            s[0] = f(0.9) * s[0] + (f(1) - f(0.9)) * g
            s[1] = f(0.999) * s[1] + (f(1) - f(0.999)) * g * g
            p = p - lr_t * s[0] / (np.sqrt(s[1]) + f(1e-8))
    return [p] + s


@pytest.mark.parametrize("kind", KERNELS)
def test_optimizer_kernel_200_steps_against_the_float64_recurrence(ops, kind):
    """200 updates with a fresh gradient each.  Bound: 4 x the error of a NumPy float32 evaluation of the same recurrence against float64
    on the same inputs (largest entry error over the largest float64 entry, per buffer) - fused multiply-adds and another evaluation
    order are legitimate.  Reference errors measured (CPU, n = 50 021): sgd p 1.07e-6; momentum p 6.6e-7, acc 2.7e-7; nesterov p 6.7e-7,
    acc 2.7e-7; adam p 7.7e-7, m 1.8e-7, v 9.1e-7 - printed by the test next to the kernel's."""
    n, steps, lr = 50021, 200, 0.01
    rs = np.random.RandomState(len(kind))
    p0 = rs.randn(n).astype(np.float32)
    gs = [rs.randn(n).astype(np.float32) for _ in range(steps)]
    nslots = {"sgd": 0, "momentum": 1, "nesterov": 1, "adam": 2}[kind]
    want = [p0.astype(np.float64)] + [np.zeros(n) for _ in range(nslots)]
    for t, g in enumerate(gs, 1):
        g64 = g.astype(np.float64)
        if kind == "sgd":
            want = [O.sgd_update(want[0], g64, lr)]
        elif kind == "adam":
            want = list(O.adam_update(want[0], g64, want[1], want[2], t, lr, B1, B2, EPS))
        else:
            want = list(O.momentum_update(want[0], g64, want[1], lr, 0.9, kind == "nesterov"))
    ref32 = _f32_recurrence(kind, p0, gs, [np.zeros(n, np.float32) for _ in range(nslots)], lr)
    bufs = [dev(p0)] + [dev(np.zeros(n)) for _ in range(nslots)]
    for t, g in enumerate(gs, 1):
        gd = dev(g)
        if kind == "sgd":
            ops.sgd_update(bufs[0], gd, lr)
        elif kind == "adam":
            ops.adam_update(bufs[0], gd, bufs[1], bufs[2], lr, t)
        else:
            ops.momentum_update(bufs[0], gd, bufs[1], lr, 0.9, kind == "nesterov")
    for name, b, w, r in zip(["p", "acc" if nslots == 1 else "m", "v"], bufs, want, ref32):
        scale = np.abs(w).max()
        ref_err = np.abs(r.astype(np.float64) - w).max() / scale
        err = np.abs(host(b) - w).max() / scale
        print("%s %s after %d steps: float32 NumPy recurrence %.3e, kernel %.3e (allowed 4 x the former)" % (kind, name, steps, ref_err, err))
        assert ref_err > 0 and err <= 4.0 * ref_err, (kind, name, err, ref_err)


def _mixed_magnitudes(n, seed):
    rs = np.random.RandomState(seed)
    return (rs.randn(n) * 10.0 ** rs.uniform(-3, 3, n)).astype(np.float32)


@pytest.mark.parametrize("n", [1000, 131073, 8 * 1024 * 1024 + 3])
@pytest.mark.parametrize("what", ["sumsq", "l2_reg_loss"])
def test_sum_of_squares_kernels(ops, what, n):
    """xv_sumsq / xv_l2_reg_loss on magnitudes 1e-3 ... 1e3 against the float64 sum: below the grid cap, one element above it, and 64
    trips round the grid-stride loop; accumulated into a zero and into a non-zero *out."""
    x = _mixed_magnitudes(n, n % 1009)
    scale = 1e-2
    factor = 1.0 if what == "sumsq" else 0.5 * scale
    ref = factor * float((x.astype(np.float64) ** 2).sum())
    report = {}
    bound = sumsq_bound(x, report)
    xd = dev(x)
    for start in (0.0, 0.37 * ref):
        acc = dev(np.array([start, SENTINEL]))
        ops.sumsq(xd, acc[:1]) if what == "sumsq" else ops.l2_reg_loss(xd, scale, acc[:1])
        got = host(acc)
        assert got[1] == SENTINEL
        want = float(np.float32(start)) + ref
        err = abs(got[0] - want) / want
        print("%s n=%d into %.3g: rel err %.3e, float32 blocked sum %.3e, bound %.3e" % (what, n, start, err, report["f32_blocked_sum_rel_err"], bound))
        assert err <= bound, (what, n, start, err, bound)
