"""The launch form of the loss head's row kernel (csrc/xv_loss.hip softmax_rows_form: margin_softmax_rows_kernel<RQ>) restated in Python
and checked against the library's own answer (xv_debug_softmax_rows_form: host arithmetic, no GPU needed) at every boundary of the rule
and at the pitches the engine uses for the speaker counts of tests/test_gpu_loss_head.py.  The GPU rows of that file use this
restatement to pin the form each of them runs."""
import ctypes

import pytest

RQ8, RQ16, THREE_PASS = 8, 16, 0
FORM_NAMES = {RQ8: "RQ=8", RQ16: "RQ=16", THREE_PASS: "RQ=0"}
BLOCK = 256                    # threads of margin_softmax_rows_kernel


def align4(n):
    return (n + 3) // 4 * 4


def rows_form(ldl, logits=0, dlogits=0):
    """softmax_rows_form, restated: the row lives in registers (RQ float4 per thread) when the pitch is a whole number of float4, both
    row bases are 16-byte aligned and the row fits 256 x RQ float4; otherwise three passes over memory."""
    if ldl % 4 or logits % 16 or dlogits % 16:
        return THREE_PASS
    nq = ldl // 4
    if nq <= BLOCK * 8:
        return RQ8
    if nq <= BLOCK * 16:
        return RQ16
    return THREE_PASS


def _lib():
    from tf_kaldi_speaker_amd import _lib as L
    return L.load()


def lib_form(ldl, logits=0, dlogits=0):
    return _lib().xv_debug_softmax_rows_form(ldl, logits, dlogits)


BASE = 0x7f0000000000          # an address as the allocator hands them out (256-byte aligned)


@pytest.mark.parametrize("ldl,want", [(4, RQ8), (8188, RQ8), (8192, RQ8), (8196, RQ16), (16380, RQ16), (16384, RQ16), (16388, THREE_PASS),
                                      (1 << 20, THREE_PASS)])
def test_pitch_boundaries(ldl, want):
    assert rows_form(ldl, BASE, BASE) == want
    assert lib_form(ldl, BASE, BASE) == want, "ldl=%d: the library runs %s, the rule says %s" % (
        ldl, FORM_NAMES.get(lib_form(ldl, BASE, BASE)), FORM_NAMES[want])


@pytest.mark.parametrize("ldl", [1, 2, 3, 5, 1001, 8191, 8193, 8194, 8195, 16383, 16385, 20011])
def test_pitch_not_a_multiple_of_four_takes_three_passes(ldl):
    assert rows_form(ldl, BASE, BASE) == THREE_PASS
    assert lib_form(ldl, BASE, BASE) == THREE_PASS


@pytest.mark.parametrize("ldl", [4, 8192, 8196, 16384])
@pytest.mark.parametrize("off_logits,off_dlogits", [(4, 0), (0, 4), (8, 0), (0, 12), (4, 4)])
def test_misaligned_rows_take_three_passes(ldl, off_logits, off_dlogits):
    assert rows_form(ldl, BASE + off_logits, BASE + off_dlogits) == THREE_PASS
    assert lib_form(ldl, BASE + off_logits, BASE + off_dlogits) == THREE_PASS
    # the same pitch at 16-byte offsets keeps the register form
    assert lib_form(ldl, BASE + 16, BASE + 48) == rows_form(ldl) != THREE_PASS


@pytest.mark.parametrize("n,want", [(7351, RQ8), (8189, RQ8), (8193, RQ16), (12289, RQ16), (16381, RQ16), (16385, THREE_PASS),
                                    (20011, THREE_PASS)])
def test_engine_pitch_of_speaker_counts(n, want):
    """The engine's logits pitch is align(N, 4) (xv_engine_head.hip, xvh_configure): VoxCeleb1+2 (7 351 speakers) keeps RQ = 8, 8 193 ... 16 384 speakers
    run RQ = 16, more than 16 384 the three-pass form."""
    ldl = align4(n)
    assert rows_form(ldl, BASE, BASE) == want
    assert lib_form(ldl, BASE, BASE) == want


def test_restatement_matches_library_over_a_grid():
    for ldl in list(range(1, 64)) + list(range(8160, 8232)) + list(range(16352, 16420)):
        for off in (0, 4, 8, 12, 16):
            assert lib_form(ldl, BASE + off, BASE) == rows_form(ldl, BASE + off, BASE), (ldl, off)
            assert lib_form(ldl, BASE, BASE + off) == rows_form(ldl, BASE, BASE + off), (ldl, off)


def test_hook_is_declared_with_pointer_width_addresses():
    from tf_kaldi_speaker_amd import _lib as L
    res, args = L.SIGNATURES["xv_debug_softmax_rows_form"]
    assert res is ctypes.c_int and ctypes.sizeof(args[1]) == ctypes.sizeof(ctypes.c_void_p) == ctypes.sizeof(args[2])
    # an address above 4 GB keeps its low bits through the call
    assert lib_form(16384, (1 << 40) + 4, 1 << 40) == THREE_PASS
    assert lib_form(16384, (1 << 40) + 16, 1 << 40) == RQ16
