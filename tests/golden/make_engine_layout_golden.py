"""Records tests/golden/engine_layout.json: what an engine's layout is for one configuration of every pooling kind and loss-head kind - the
variable table, the counts, the stage gradient ranges, the arena size and where the endpoints lie in the arena.

Run on an MI355X at the commit whose layout is to be pinned:  python tests/golden/make_engine_layout_golden.py
Only the C ABI is used (tf_kaldi_speaker_amd/_lib.py), so the same script records any tree with the same ABI version;
tests/test_gpu_engine_layout.py imports CONFIGS and record() from here and asserts equality with the file.

Small capacities (max_batch 4, max_frames 24, 40 speakers) with the shipped layer widths.  The endpoint call wants a forward first (it
reports the rows of the most recent one): one inference forward of 2 x 24 zero frames on zero variables.  Endpoints are recorded as byte
offsets from tdnn1_conv, the first layer's pre-BN tensor; the ones that do not lie in the arena (the `_bn` scratch, vlad_centers in the
variable buffer) are left out.
"""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "engine_layout.json")
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

EXTENDED = ((5, 512), (1, 512), (3, 512), (1, 512), (3, 512), (1, 512), (3, 512), (1, 512), (1, 512), (1, 1500))
BASE = dict(feat_dim=30, num_speakers=40, num_nodes_pooling_layer=1500, num_nodes_last_layer=512, feature_scaling_factor=1.0, lambda_base=1000.0,
            lambda_gamma=1e-4, lambda_power=5.0, weight_l2_regularizer=1e-2, output_weight_l2_regularizer=-1.0, batchnorm_momentum=0.99,
            bn_epsilon=1e-3, fused_bn_unbiased_moving_var=1, momentum=0.9, max_batch=4, max_frames=24, ring_loss_init=20.0, ring_loss_lambda=0.01,
            mhe_lambda=0.01)
ATT = dict(pooling=1, att_key0_nodes=1500, att_key1_nodes=1500, att_use_scale=1)
AM = dict(loss_kind=2, margin_m=0.2)
# name -> the xv_config fields on top of BASE ("frame_layers" and "pair" are spelt out by config() / record())
CONFIGS = {
    "statistics_softmax": dict(),
    "attention_key0_amsoftmax_f32": dict(ATT, att_key_type=0, **AM),
    "attention_key0_amsoftmax_f16x3": dict(ATT, att_key_type=0, precision=1, **AM),
    "attention_key2_amsoftmax_f32": dict(ATT, att_key_type=2, optimizer=1, **AM),
    "attention_key2_amsoftmax_f16x3": dict(ATT, att_key_type=2, precision=1, **AM),
    "ghost_vlad_asoftmax_ring_mhe": dict(pooling=2, vlad_num_centers=8, vlad_num_ghosts=2, loss_kind=1, margin_m=4.0, aux_ring=1, aux_mhe=1, optimizer=2),
    "statistics_semihard_triplet": dict(loss_kind=4, pair=dict(kind=0)),
    "attention_angular_triplet": dict(ATT, att_key_type=3, loss_kind=5, pair=dict(kind=1, margin_kind=2, margin=0.2, valid_speakers=2, valid_segments=2)),
    "extended_asoftmax": dict(loss_kind=1, margin_m=4.0, lambda_min=10.0, frame_layers=EXTENDED),
    "predict_only_max_rows": dict(num_speakers=0, max_rows=48),
    "prelu_softmax": dict(relu_type=1),
}
ENDPOINTS = (["tdnn%d_%s" % (i, k) for i in range(1, 13) for k in ("conv", "dense", "relu")]
             + ["att_key0_dense", "att_key0_relu", "att_key1_dense", "att_key1_relu", "attention_weights", "vlad_key", "vlad_weights", "pooling",
                "output", "logits", "debug:dpool"])


def config(_lib, fields):
    fields = dict(BASE, **fields)
    fields.pop("pair", None)
    table = fields.pop("frame_layers", None)
    c = _lib.XvConfig(**fields)
    if table:
        c.num_frame_layers = len(table)
        for i, (k, w) in enumerate(table):
            c.frame_context[i], c.frame_width[i] = k, w
    return c


def record(name):
    """The layout of configuration `name` as a JSON-ready dict."""
    import torch
    from tf_kaldi_speaker_amd import _lib
    lib = _lib.load()
    cfg, h = config(_lib, CONFIGS[name]), C.c_void_p()
    _lib.check(lib.xv_engine_create(C.byref(cfg), C.byref(h)), "xv_engine_create")
    try:
        pair = CONFIGS[name].get("pair")
        if pair:
            _lib.check(lib.xv_engine_set_pair_loss(h, C.byref(_lib.XvPairLossConfig(**pair))), "xv_engine_set_pair_loss")
        out = {"variables": [], "arena_bytes": int(lib.xv_engine_arena_bytes(h)),
               "counts": [int(lib.xv_engine_variables_count(h)), int(lib.xv_engine_trainable_count(h)), int(lib.xv_engine_optimizer_state_count(h))]}
        for i in range(lib.xv_engine_num_variables(h)):
            vname, shape, rank, off, tr = C.c_char_p(), (C.c_int32 * 4)(), C.c_int32(), C.c_size_t(), C.c_int32()
            _lib.check(lib.xv_engine_variable_info(h, i, C.byref(vname), shape, C.byref(rank), C.byref(off), C.byref(tr)), "xv_engine_variable_info")
            out["variables"].append([vname.value.decode(), list(shape)[:rank.value], int(tr.value), int(off.value)])
        out["stages"] = []
        for st in range(_lib.XV_BWD_STAGES):
            b, e = C.c_size_t(), C.c_size_t()
            _lib.check(lib.xv_engine_stage_grad_range(h, st, C.byref(b), C.byref(e)), "xv_engine_stage_grad_range")
            out["stages"].append([int(b.value), int(e.value)])
        dev = torch.device("cuda:0")
        variables = torch.zeros(out["counts"][0], dtype=torch.float32, device=dev)
        feats = torch.zeros(2 * 24 * 30, dtype=torch.float32, device=dev)
        _lib.check(lib.xv_engine_bind(h, variables.data_ptr(), None, None), "xv_engine_bind")
        _lib.check(lib.xv_engine_forward(h, None, feats.data_ptr(), 2, 24, 0), "xv_engine_forward")
        found = {}
        for ep in ENDPOINTS:
            p, rows, cols, ld = C.c_void_p(), C.c_int32(), C.c_int32(), C.c_int32()
            if lib.xv_engine_endpoint(h, ep.encode(), C.byref(p), C.byref(rows), C.byref(cols), C.byref(ld)) == 0:
                found[ep] = [p.value, rows.value, cols.value, ld.value]
        torch.cuda.synchronize()
        base = found["tdnn1_conv"][0]
        out["endpoints"] = {ep: [v[0] - base] + v[1:] for ep, v in found.items()}
        return out
    finally:
        lib.xv_engine_destroy(h)


if __name__ == "__main__":
    golden = {name: record(name) for name in CONFIGS}
    with open(sys.argv[1] if len(sys.argv) > 1 else PATH, "w") as f:
        json.dump(golden, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %d configurations, %d variables, %d endpoints" % (len(golden), sum(len(g["variables"]) for g in golden.values()),
                                                                    sum(len(g["endpoints"]) for g in golden.values())))
