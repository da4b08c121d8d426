"""Loss functions with the reference's signatures.  The softmax family (model/loss.py:9,51,172,260):

    f(features[B,E], labels[B], num_outputs, params, is_training=None, reuse_variables=None, name="softmax")
        -> (loss, endpoints{"logits", "labels"})        side effect: params.dict["softmax_w"] = w

These are the *forward* (evaluation) forms on GPU buffers; gradients of the same kernels are
produced inside the engine (csrc/xv_engine_fwd.hip: xv_engine_loss_forward; its gradient: csrc/xv_engine_bwd.hip)
that Trainer drives.  Variables live in a module-level store keyed by "<name>/output/kernel" exactly like the TF variable scope, so a second call with
reuse_variables=True sees the same weight (loss.py:96-102; model/common.VariableStore).  The four functions are one body on the kind's record
(kinds.py: code, margin prefix, the margins it takes).

The pairwise heads (loss.py:358-705) have no variables: semihard_triplet_loss, angular_triplet_loss and e2e_valid_loss return
(loss, endpoints{"loss", "labels"}) from csrc/xv_triplet.hip; their gradient is ops.pair_loss_backward, and the engine's stage 0.
ge2e_loss (loss.py:903-982) has the two scalars "<name>/w" and "<name>/b" in the same store; its gradient is ops.ge2e_loss_backward.
"""
from collections import OrderedDict

import torch

try:
    from .. import ops, kinds
    from .common import to_device, shape_list, VariableStore
except (ImportError, ValueError):
    import ops
    import kinds
    from model.common import to_device, shape_list, VariableStore

_STORE = VariableStore(lambda v: to_device(v), getter="get_variable()")
_VARIABLES = _STORE.variables      # name -> torch tensor (device)
reset_variables, set_variable = _STORE.reset, _STORE.preset


def get_variable(name, shape, reuse, init="xavier"):
    """tf.get_variable under tf.variable_scope(reuse=reuse).  init: "xavier" / "zeros" (what kinds.initial_value gives this name: the
    output kernel, loss.py:100-102; its bias) or the constant (the ring loss's r, loss.py:1009-1011)."""
    return _STORE.get(name, shape, create=reuse is not True, reuse=bool(reuse), constant=init if isinstance(init, float) else None)


def _lambda(params, prefix):
    lmin = float(params.dict[prefix + "_lambda_min"])
    base = float(params.dict[prefix + "_lambda_base"])
    gamma = float(params.dict[prefix + "_lambda_gamma"])
    power = float(params.dict[prefix + "_lambda_power"])
    params.dict[prefix + "_lambda_min"], params.dict[prefix + "_lambda_base"] = lmin, base
    params.dict[prefix + "_lambda_gamma"], params.dict[prefix + "_lambda_power"] = gamma, power
    step = float(params.dict.get("global_step", 0))
    return max(lmin, base * (1.0 + gamma * step) ** (-power))      # loss.py:144-145


def _run(kind, features, labels, num_outputs, params, reuse_variables, name, m, lam):
    """kind: the record of a loss of the softmax family (kinds.py); plain softmax has the bias, the margin kinds normalise the weights."""
    x = to_device(features)
    y = to_device(labels, torch.int32)
    assert len(shape_list(x)) == len(shape_list(y)) + 1
    e = x.shape[1]
    w = get_variable(name + "/output/kernel", (e, num_outputs), reuse_variables)
    params.dict["softmax_w"] = w
    normalized = kind.prefix is not None
    bias = None if normalized else get_variable(name + "/output/bias", (num_outputs,), reuse_variables, init="zeros")
    inv, wn, wnt = ops.loss_prep_weight(w, normalized)
    ldl = wn.shape[1]
    logits = torch.zeros((x.shape[0], ldl), dtype=torch.float32, device=x.device)
    logits[:, :num_outputs] = ops.affine_forward(x.view(x.shape[0], 1, e), 1, wnt, bias, num_outputs)
    loss, _, _, _ = ops.margin_softmax_rows(kind.code, logits, num_outputs, x, y, m, lam)
    endpoints = OrderedDict()
    endpoints["logits"] = logits[:, :num_outputs]
    endpoints["labels"] = y
    total = loss[0]
    aux_funcs = params.dict.get("aux_loss_func") or []
    if kind.integer_margins and m == 1.0:       # asoftmax, m = 1: the reference returns before the auxiliary losses (loss.py:110-115)
        aux_funcs = []
    ring, mhe = kinds.AUX_LOSSES
    for aux in aux_funcs:            # loss.py:985-1036, added by every other loss function (loss.py:40,161,249,347)
        if aux == ring:
            r = get_variable(name + "_ringloss/r", (), reuse_variables, init=float(params.ring_loss_init))
            total = total + ops.ring_loss(x, r, float(params.ring_loss_lambda))
            endpoints["ring_loss_r"] = r
        elif aux == mhe:
            wn_unit = wn if normalized else ops.loss_prep_weight(w, True)[1]      # MHE normalises the weights itself (loss.py:1026)
            total = total + ops.mhe_loss(wn_unit, num_outputs, y, float(params.mhe_lambda))
            endpoints["w"] = w
        else:
            raise NotImplementedError("Unsupported loss function %s" % aux)
    return total, endpoints


def _margin(kind, params):
    """The kind's margin from params.<prefix>_m; a real-valued one is written back as a float (loss.py:196,284)."""
    key = kind.prefix + "_m"
    if kind.integer_margins:
        m = int(getattr(params, key))
        if m not in kind.integer_margins:
            raise NotImplementedError("[ERROR] m=%d is not unsupported." % m)
        return float(m)
    setattr(params, key, float(getattr(params, key)))
    return getattr(params, key)


def _softmax_family(kind):
    def loss(features, labels, num_outputs, params, is_training=None, reuse_variables=None, name="softmax"):
        if kind.prefix is None:
            return _run(kind, features, labels, num_outputs, params, reuse_variables, name, 0.0, 0.0)
        return _run(kind, features, labels, num_outputs, params, reuse_variables, name, _margin(kind, params), _lambda(params, kind.prefix))
    loss.__name__ = kind.name
    return loss


# loss.py:9,51,172,260, in the records' order; then the records of the two pairwise heads
softmax, asoftmax, additive_margin_softmax, additive_angular_margin_softmax = (
    _softmax_family(k) for k in kinds.LOSSES.values() if k.family == kinds.SOFTMAX)
_SEMIHARD, _ANGULAR = (k for k in kinds.LOSSES.values() if k.family == kinds.PAIR)


def _embeddings(features, labels):
    x = to_device(features)
    y = to_device(labels, torch.int32)
    assert len(shape_list(x)) == len(shape_list(y)) + 1
    return x, y


def _pair_endpoints(loss, y, stats=None):
    endpoints = OrderedDict()
    endpoints["loss"] = loss[0]
    endpoints["labels"] = y
    if stats is not None:
        endpoints["stats"] = stats
    return loss[0], endpoints


def semihard_triplet_loss(features, labels, num_outputs, params, is_training=None, reuse_variables=None, name="triplet_loss"):
    """loss.py:358-498; params.margin, params.triplet_loss_squared.  -> (loss, endpoints{"loss", "labels", "stats"})"""
    x, y = _embeddings(features, labels)
    cfg = ops.pair_loss_config(_SEMIHARD.name, margin=float(params.margin), squared=params.triplet_loss_squared)
    loss, stats, _ = ops.pair_loss(cfg, x, y)
    return _pair_endpoints(loss, y, stats)


def angular_triplet_loss(features, labels, num_outputs, params, is_training=None, reuse_variables=None, name="angular_triplet_loss"):
    """loss.py:501-634; params.margin, params.triplet_type ("all", "hard"), params.loss_type (the margin on the positive side)."""
    x, y = _embeddings(features, labels)
    kinds.check_angular(params.triplet_type, params.loss_type)
    params.margin = float(params.margin)
    cfg = ops.pair_loss_config(_ANGULAR.name, margin=params.margin, triplet_type=params.triplet_type, loss_type=params.loss_type)
    loss, stats, _ = ops.pair_loss(cfg, x, y)
    return _pair_endpoints(loss, y, stats)


def e2e_valid_loss(features, labels, num_outputs, params, is_training=None, reuse_variables=None, name="valid_e2e_loss"):
    """loss.py:637-705: the features are arranged by speaker, params.num_valid_speakers_per_batch x params.num_valid_segments_per_speaker."""
    x, y = _embeddings(features, labels)
    assert "num_valid_speakers_per_batch" in params.dict and "num_valid_segments_per_speaker" in params.dict, \
        "Valid parameters should be set if E2E loss is selected"
    loss = ops.e2e_valid_loss(x, int(params.num_valid_speakers_per_batch), int(params.num_valid_segments_per_speaker))
    return _pair_endpoints(loss, y)


def ge2e_loss(features, labels, num_outputs, params, is_training=None, reuse_variables=None, name="ge2e"):
    """loss.py:903-982: the features are arranged by speaker, params.num_speakers_per_batch x params.num_segments_per_speaker; labels are not
    read.  params.ge2e_loss_type ("softmax", "contrastive"); the variables "<name>/w" and "<name>/b" start from params.init_end2end_w and
    params.init_end2end_b.  -> (loss, endpoints{"loss", "labels", "stats", "w", "b"})"""
    x, y = _embeddings(features, labels)
    w = get_variable(name + "/w", (), reuse_variables, init=float(params.init_end2end_w))
    b = get_variable(name + "/b", (), reuse_variables, init=float(params.init_end2end_b))
    cfg = ops.ge2e_loss_config(params.ge2e_loss_type, int(params.num_speakers_per_batch), int(params.num_segments_per_speaker))
    loss, stats, _ = ops.ge2e_loss(cfg, x, w.reshape(1), b.reshape(1))
    total, endpoints = _pair_endpoints(loss, y, stats)
    endpoints["w"], endpoints["b"] = w, b
    return total, endpoints


def generalized_angular_triplet_loss(*a, **k):
    raise NotImplementedError("generalized_angular_triplet_loss (the centre-based triplet loss with a [batch, num_speakers] distance matrix and a "
                              "moving-average centre update, loss.py:708) is not implemented; semihard_triplet_loss and angular_triplet_loss are")
