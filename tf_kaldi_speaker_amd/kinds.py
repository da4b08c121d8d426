"""What the Python layer knows about a pooling kind and about a loss kind, one record each; the initial value of a variable.

A record holds, for its kind and nothing else: the ABI code (_lib), the options it reads from a params dict and the engine.make_config
keywords they become (`keywords`), how make_config writes those into XvConfig with the numeric checks it makes there (`write`), the reference
options it refuses by name - `refuse(d, last_relu)` with the engine's frame layers, `refuse(d)` in the op-level form of model/pooling.py -
and, for a pooling kind, its endpoint names and the params prefixes that belong in tdnn()'s graph key.  A condition that two refusal sites
state is evaluated by one function here; each site keeps its own wording.  The C library checks the numbers again: it is the authority for the ABI.

Readers: engine.make_config, ops.pair_loss_config, ops.ge2e_loss_config, model/tdnn.py, model/loss.py, model/pooling.py, model/trainer.py.  None of them compares
against a kind's name.  A new kind is a record here, its code in _lib.py and its C unit ("Adding a kind").
"""
from collections import OrderedDict
from types import SimpleNamespace as Kind      # a record: the attributes given, nothing else

import numpy as np

try:
    from . import _lib
except ImportError:      # drop-in layout: PYTHONPATH=$TF_KALDI_ROOT makes these top-level modules
    import _lib


# ---- pooling kinds ------------------------------------------------------------------------------------------------------------------
def _none(*a, **k):
    return {}


def _bad_key_type(key_type):
    return int(key_type) not in (0, 1, 2, 3)


def _attention_refuse(d, last_relu=None):
    """model/pooling.py:37-192 in the form the shipped attention configs use; everything else the function offers (value network, several
    heads, split keys, penalty term, post non-linearity) is refused by name.  last_relu "tdnn<F>_relu": the engine form - key = the
    last-but-one frame layer, value = the last, two key layers, all faults in one message; None: the op-level form, which takes any
    endpoints and any number of key layers and names its first fault."""
    faults = dict(value_network=len(d.get("att_value_num_nodes", [])) != 0,      # the conditions that both forms state
                  heads=int(d.get("att_num_heads", 1)) != 1 or bool(d.get("att_split_key", False)),
                  penalty=float(d.get("att_penalty_term", 0) or 0) != 0.0,
                  nonlinear=bool(d.get("att_apply_nonlinear", False)))
    relu = d.get("network_relu_type", "relu")
    if last_relu is None:
        if relu != "relu":
            raise NotImplementedError("self_attention: network_relu_type %r (relu only)" % d.get("network_relu_type"))
        for fault, text in (("value_network", "no value network (att_value_num_nodes must be empty)"), ("heads", "one head, key not split"),
                            ("nonlinear", "att_apply_nonlinear is not supported"), ("penalty", "att_penalty_term must be 0 (one head has no penalty)")):
            if faults[fault]:
                raise NotImplementedError("self_attention on the MI355X kernels: " + text)
        if len(d["att_key_num_nodes"]) < 1:
            raise NotImplementedError("self_attention: att_key_num_nodes needs at least the key layer")
        if _bad_key_type(d["att_key_network_type"]):
            raise NotImplementedError("self_attention: att_key_network_type %r is not one of 0..3" % int(d["att_key_network_type"]))
        return
    nf = int(last_relu[4:-5])
    key_type = int(d.get("att_key_network_type", -1))
    unsupported = [text for bad, text in (
        (d.get("att_key_input") != "tdnn%d_relu" % (nf - 1), "att_key_input=%r (tdnn%d_relu)" % (d.get("att_key_input"), nf - 1)),
        (d.get("att_value_input") != last_relu, "att_value_input=%r (%s)" % (d.get("att_value_input"), last_relu)),
        (faults["value_network"], "att_value_num_nodes (no value network)"),
        (len(d.get("att_key_num_nodes", [])) != 2, "att_key_num_nodes (two key layers)"),
        (_bad_key_type(key_type), "att_key_network_type=%r (0..3)" % d.get("att_key_network_type")),
        (key_type == 1 and relu != "relu", "att_key_network_type 1 with network_relu_type %s (the score kernel's fused ReLU is a plain one)" % relu),
        (faults["heads"], "att_num_heads / att_split_key (one head)"),
        (faults["penalty"], "att_penalty_term (0)"),
        (faults["nonlinear"], "att_apply_nonlinear (false)")) if bad]
    if unsupported:
        raise NotImplementedError("self_attention on the MI355X engine supports the shipped single-head form only; not: " + ", ".join(unsupported))


def _attention_keywords(d):
    return dict(att_key_num_nodes=tuple(d["att_key_num_nodes"]), att_key_network_type=int(d["att_key_network_type"]),
                att_use_scale=bool(d.get("att_use_scale", False)))


def _attention_write(c, kw):
    # the shipped single-head form (nnet_conf/*_tdnn4_att.json): two key layers on tdnn4_relu, value = tdnn5_relu
    nodes, key_type = kw["att_key_num_nodes"], kw["att_key_network_type"]
    if len(nodes) != 2:
        raise NotImplementedError("self_attention: att_key_num_nodes must have two entries (dense+bn+relu, then the key layer)")
    if _bad_key_type(key_type):
        raise NotImplementedError("self_attention: att_key_network_type %r is not one of 0..3 (pooling.py:84-96)" % key_type)
    c.att_key0_nodes, c.att_key1_nodes = int(nodes[0]), int(nodes[1])
    c.att_key_type = int(key_type)
    c.att_use_scale = int(bool(kw["att_use_scale"]))


def _bad_clusters(k, g):
    return k < 1 or g < 0 or k + g > 64


def _vlad_refuse(d, last_relu=None):
    """The ghost_vlad options the kernels cover (pooling.py:195-277 without key / value networks), the rest refused by name.  last_relu: the
    only endpoint the engine can pool ("tdnn5_relu"); None (the op-level function) takes any endpoint.  -> (centres, ghosts)"""
    unsupported = []
    if len(d.get("vlad_key_num_nodes", [])) != 0:
        unsupported.append("vlad_key_num_nodes (no key network)")
    if len(d.get("vlad_value_num_nodes", [])) != 0:
        unsupported.append("vlad_value_num_nodes (no value network)")
    for key in ("vlad_key_input", "vlad_value_input"):
        if last_relu is not None and d.get(key) != last_relu:
            unsupported.append("%s=%r (%s)" % (key, d.get(key), last_relu))
    if d.get("vlad_key_input") != d.get("vlad_value_input"):
        unsupported.append("vlad_key_input != vlad_value_input (one tensor is key and value)")
    k, g = int(d.get("vlad_num_centers", 0)), int(d.get("vlad_num_ghosts", 0))
    if _bad_clusters(k, g):
        unsupported.append("vlad_num_centers=%d, vlad_num_ghosts=%d (at least one centre, at most 64 clusters)" % (k, g))
    if d.get("precision", "f32") not in (None, "f32"):
        unsupported.append("precision %s (f32)" % d["precision"])
    if unsupported:
        raise NotImplementedError("ghost_vlad on the MI355X kernels: not " + ", ".join(unsupported))
    return k, g


def _vlad_keywords(d):
    return dict(vlad_num_centers=int(d["vlad_num_centers"]), vlad_num_ghosts=int(d.get("vlad_num_ghosts", 0)),
                vlad_final_l2_norm=bool(d.get("vlad_final_l2_norm", False)))


def _vlad_write(c, kw):
    k, g = int(kw["vlad_num_centers"]), int(kw["vlad_num_ghosts"])
    if _bad_clusters(k, g):
        raise NotImplementedError("ghost_vlad: vlad_num_centers >= 1, vlad_num_ghosts >= 0 and at most 64 clusters in all (got %d + %d)" % (k, g))
    if kw["precision"] != "f32":
        raise NotImplementedError("ghost_vlad: precision %s is not supported (f32 only)" % kw["precision"])
    c.vlad_num_centers, c.vlad_num_ghosts, c.vlad_final_l2_norm = k, g, int(bool(kw["vlad_final_l2_norm"]))


def _pooling(name, keywords=_none, write=_none, refuse=_none, endpoints=(), key_prefixes=()):
    return Kind(name=name, code=_lib.POOLINGS[name], keywords=keywords, write=write, refuse=refuse, endpoints=endpoints, key_prefixes=key_prefixes)


# in the order their endpoints take in tdnn.endpoint_order (pooling.py:78-149; :250,273-275 - vlad_value is tdnn<F>_relu)
POOLINGS = OrderedDict((k.name, k) for k in (
    _pooling("statistics_pooling"),
    _pooling("self_attention", _attention_keywords, _attention_write, _attention_refuse, key_prefixes=("att_",),
             endpoints=("att_key0_dense", "att_key0_bn", "att_key0_relu", "att_key1_dense", "att_key1_bn", "att_key1_relu", "attention_weights")),
    _pooling("ghost_vlad", _vlad_keywords, _vlad_write, _vlad_refuse, key_prefixes=("vlad_",),
             endpoints=("vlad_weights", "vlad_key", "vlad_centers", "pooling"))))
assert set(POOLINGS) == set(_lib.POOLINGS)


def pooling(name):
    if name not in POOLINGS:
        raise NotImplementedError("Not implement %s pooling" % name)
    return POOLINGS[name]


# ---- loss kinds ---------------------------------------------------------------------------------------------------------------------
SOFTMAX, PAIR, GE2E, REFUSED = "softmax family", "pairwise head", "GE2E head", "refused"
HEADS_WITHOUT_SPEAKERS = (PAIR, GE2E)      # no softmax/output variables: configured whatever num_speakers says; validated on end2end batches


def _margin_keywords(prefix):
    def keywords(d):
        return dict(margin_m=float(d[prefix + "_m"]), lambda_min=float(d[prefix + "_lambda_min"]), lambda_base=float(d[prefix + "_lambda_base"]),
                    lambda_gamma=float(d[prefix + "_lambda_gamma"]), lambda_power=float(d[prefix + "_lambda_power"]))
    return keywords


def check_angular(triplet_type, loss_type):
    """The asserts of loss.py:518-519, for every site that takes the angular loss's options."""
    assert triplet_type == "all" or triplet_type == "hard"
    assert loss_type in MARGINS


def _pair_keywords(d):
    # trainer.py:234-250; aux_loss_func travels so that make_config can say that it drops it
    return dict(margin=float(d["margin"]), aux_loss_func=tuple(d.get("aux_loss_func") or ()))


def _semihard_keywords(d):
    return dict(_pair_keywords(d), triplet_loss_squared=bool(d["triplet_loss_squared"]))


def _angular_keywords(d):      # with the asserts of loss.py:518-519; the validation layout: loss.py:657-658
    check_angular(d["triplet_type"], d["loss_type"])
    assert "num_valid_speakers_per_batch" in d and "num_valid_segments_per_speaker" in d, "Valid parameters should be set if E2E loss is selected"
    return dict(_pair_keywords(d), triplet_type=d["triplet_type"], loss_type=d["loss_type"],
                num_valid_speakers_per_batch=int(d["num_valid_speakers_per_batch"]),
                num_valid_segments_per_speaker=int(d["num_valid_segments_per_speaker"]))


def _angular_check(margin, triplet_type, loss_type):
    check_angular(triplet_type, loss_type)
    if MARGINS[loss_type].integer_margins and int(margin) not in MARGINS[loss_type].integer_margins:
        raise NotImplementedError("[ERROR] m=%d is not unsupported if %s is selected." % (margin, loss_type))


def check_ge2e(ge2e_loss_type, num_segments_per_speaker):
    """The assert of loss.py:937 and the ValueError of loss.py:980, for every site that takes the GE2E loss's options."""
    assert int(num_segments_per_speaker) != 1
    if ge2e_loss_type not in _lib.GE2E_TYPES:
        raise ValueError("The GE2E only support softmax and contrastive loss")


def _ge2e_keywords(d):      # loss.py:916-936; the validation layout: loss.py:657-658
    check_ge2e(d["ge2e_loss_type"], d["num_segments_per_speaker"])
    assert "num_valid_speakers_per_batch" in d and "num_valid_segments_per_speaker" in d, "Valid parameters should be set if E2E loss is selected"
    return dict(ge2e_loss_type=d["ge2e_loss_type"], init_end2end_w=float(d["init_end2end_w"]), init_end2end_b=float(d["init_end2end_b"]),
                num_speakers_per_batch=int(d["num_speakers_per_batch"]), num_segments_per_speaker=int(d["num_segments_per_speaker"]),
                num_valid_speakers_per_batch=int(d["num_valid_speakers_per_batch"]),
                num_valid_segments_per_speaker=int(d["num_valid_segments_per_speaker"]), aux_loss_func=tuple(d.get("aux_loss_func") or ()))


def _loss(name, family, prefix=None, keywords=_none, integer_margins=None, check=_none):
    """prefix: of the margin options in a params dict ("amsoftmax" -> amsoftmax_m, amsoftmax_lambda_min, ...); integer_margins: the only
    margins the kind takes; check: what the kind's op-level config refuses - check(margin, triplet_type, loss_type) in ops.pair_loss_config
    for a pairwise head, check(ge2e_loss_type, num_segments_per_speaker) in ops.ge2e_loss_config for the GE2E head."""
    return Kind(name=name, family=family, code=_lib.LOSS_KINDS.get(name), pair_code=_lib.PAIR_KINDS.get(name), prefix=prefix,
                keywords=_margin_keywords(prefix) if prefix else keywords, integer_margins=integer_margins, check=check)


LOSSES = OrderedDict((k.name, k) for k in (
    _loss("softmax", SOFTMAX),
    _loss("asoftmax", SOFTMAX, "asoftmax", integer_margins=(1, 2, 4)),
    _loss("additive_margin_softmax", SOFTMAX, "amsoftmax"),
    _loss("additive_angular_margin_softmax", SOFTMAX, "arcsoftmax"),
    _loss("semihard_triplet_loss", PAIR, keywords=_semihard_keywords),
    _loss("angular_triplet_loss", PAIR, keywords=_angular_keywords, check=_angular_check),
    _loss("ge2e_loss", GE2E, keywords=_ge2e_keywords, check=check_ge2e),
    # the centre-based triplet loss (loss.py:708): named so that its refusal can say what it is
    _loss("generalized_angular_triplet_loss", REFUSED)))
MARGINS = OrderedDict((n, k) for n, k in LOSSES.items() if k.prefix)      # the kinds that put a margin on the target: the values of loss_type
assert set(_lib.LOSS_KINDS) == set(n for n, k in LOSSES.items() if k.family != REFUSED)
assert set(_lib.PAIR_KINDS) == set(n for n, k in LOSSES.items() if k.family == PAIR)


def loss(name, family=None):
    """The record of an implemented loss kind (of `family`, if given)."""
    k = LOSSES.get(name)
    if k is None or k.family == REFUSED or (family is not None and k.family != family):
        raise NotImplementedError("Not implement %s loss" % name)
    return k


def family(name):
    return LOSSES[name].family if name in LOSSES else None


# auxiliary to the softmax family (loss.py:985-1036; every loss function adds them, loss.py:40,161,249,347):
# name -> (XvConfig flag, its options - floats, under one name in a params dict, as make_config keywords and in XvConfig)
AUX_LOSSES = OrderedDict((("ring_loss", ("aux_ring", ("ring_loss_init", "ring_loss_lambda"))), ("mhe_loss", ("aux_mhe", ("mhe_lambda",)))))


def aux_keywords(d):
    kw = dict(aux_loss_func=tuple(d["aux_loss_func"]))
    for name, (_, options) in AUX_LOSSES.items():
        if name in d["aux_loss_func"]:
            kw.update((o, float(d[o])) for o in options)
    return kw


def write_aux(c, aux_loss_func):
    for aux in aux_loss_func:
        if aux not in AUX_LOSSES:
            raise NotImplementedError("Unsupported loss function %s" % aux)
    for name, (flag, _) in AUX_LOSSES.items():
        setattr(c, flag, int(name in aux_loss_func))


# ---- variables ----------------------------------------------------------------------------------------------------------------------
# leaf of a variable's name -> constant initial value; the leaves with a random one are named in initial_value(), everything else is 0
# ([TF] defaults of tf.layers.conv2d / dense / batch_normalization; alpha: tf.constant_initializer(0.01), common.py:37)
_CONSTANT_LEAVES = {"gamma": 1.0, "moving_variance": 1.0, "alpha": 0.01}


def initial_value(leaf, shape, rs, constant=None):
    """The initial float32 array of the variable whose name ends in `leaf`, drawing from the numpy RandomState `rs` where it is random.
    constant: the value where the configuration gives one - the ring loss's radius "r" (ring_loss_init, loss.py:1009-1011), the GE2E
    loss's "w" and "b" (init_end2end_w, init_end2end_b, loss.py:923-924)."""
    shape = tuple(shape)
    if constant is not None:
        return np.full(shape, constant, np.float32)
    if leaf in ("kernel", "vlad_centers"):      # Glorot-uniform: xavier_initializer(), loss.py:100-102, pooling.py:253-255
        fan_in, fan_out = (shape[1] * shape[2], shape[1] * shape[3]) if len(shape) == 4 else shape
        lim = np.sqrt(6.0 / (fan_in + fan_out))
        return rs.uniform(-lim, lim, size=shape).astype(np.float32)
    if leaf == "query":      # truncated_normal(stddev=0.1), pooling.py:131-132
        return np.clip(rs.randn(*shape) * 0.1, -0.2, 0.2).astype(np.float32)
    return np.full(shape, _CONSTANT_LEAVES.get(leaf, 0.0), np.float32)
