"""The arena of a predict-only engine: no loss head, no backward pass - no dz slot per layer."""
import pytest

pytestmark = pytest.mark.gpu


def test_predict_only_engine_keeps_the_two_slot_arena():
    """an engine without a loss head never runs a backward pass - it must not pay for a dz slot per layer (Trainer.predict_batch
    builds one with 49 152 rows: nine slots of 296 MB against two)."""
    from tf_kaldi_speaker_amd import engine as E
    rows = 49152
    pred = E.Engine(E.make_config(30, 0, max_batch=128, max_frames=4000, max_rows=rows), device="cuda:0")
    train = E.Engine(E.make_config(30, 100, max_batch=128, max_frames=4000, max_rows=rows), device="cuda:0")
    slot = rows * 1504 * 4
    assert train.arena_bytes - pred.arena_bytes > 5 * slot, (train.arena_bytes, pred.arena_bytes)
    assert pred.arena_bytes < 4e9, pred.arena_bytes
    pred.close(); train.close()


def _endpoint_extents(eng, names):
    """{name: (first byte, one past the last byte)} of the endpoints the engine knows among `names`, read through the C-ABI."""
    import ctypes as C
    out = {}
    for name in names:
        p, rows, cols, ld = C.c_void_p(), C.c_int32(), C.c_int32(), C.c_int32()
        if eng.lib.xv_engine_endpoint(eng.h, name.encode(), C.byref(p), C.byref(rows), C.byref(cols), C.byref(ld)) != 0:
            continue      # not an endpoint of this configuration (attention names without attention, ...)
        assert p.value and rows.value > 0 and ld.value >= cols.value > 0, (name, p.value, rows.value, cols.value, ld.value)
        out[name] = (p.value, p.value + 4 * ((rows.value - 1) * ld.value + cols.value))
    return out


@pytest.mark.parametrize("pooling", ["statistics_pooling", "self_attention"])
@pytest.mark.parametrize("precision", ["f32", "f16x3"])
def test_endpoints_lie_in_the_arena_and_do_not_overlap(precision, pooling):
    """What the arena's single layout walk must keep true: after one forward every endpoint the engine can name (the on-demand `_bn`
    scratch aside: an allocation of its own) lies in the arena, and the layers' pre-BN tensors, the pooled vector, the output and the logits
    do not overlap given their rows x ld extents.  The arena's base is not part of the C-ABI, so "in the arena" is checked as: all endpoints
    together span no more than arena_bytes."""
    import numpy as np
    from tf_kaldi_speaker_amd import engine as E
    eng = E.Engine(E.make_config(30, 16, max_batch=4, max_frames=40, precision=precision, pooling_type=pooling, att_key_num_nodes=(64, 64)),
                   device="cuda:0")
    eng.init_variables(seed=1)
    eng.forward(np.random.RandomState(0).randn(4, 40, 30).astype(np.float32), training=True)
    layers = ["tdnn%d_%s" % (i, k) for i in range(1, 8) for k in ("conv", "dense")] + ["att_key0_dense", "att_key1_dense"]
    disjoint = _endpoint_extents(eng, layers + ["pooling", "output", "logits"])
    assert len(disjoint) == (12 if pooling == "self_attention" else 10), sorted(disjoint)
    named = dict(disjoint)
    named.update(_endpoint_extents(eng, ["tdnn%d_relu" % i for i in range(1, 8)] + ["att_key0_relu", "attention_weights"]))
    assert len(named) == len(disjoint) + (9 if pooling == "self_attention" else 7), sorted(named)
    span = max(hi for _, hi in named.values()) - min(lo for lo, _ in named.values())
    assert span <= eng.arena_bytes, (span, eng.arena_bytes)
    order = sorted(disjoint.items(), key=lambda kv: kv[1][0])
    for (na, (_, hi)), (nb, (lo, _)) in zip(order, order[1:]):
        assert hi <= lo, "%s [.. %#x) overlaps %s [%#x ..)" % (na, hi, nb, lo)
    eng.close()
