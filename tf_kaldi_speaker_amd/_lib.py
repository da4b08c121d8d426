"""ctypes binding of the C-ABI declared in include/xvector_hip.h.

The shared library is the product; there is NO CPU fallback.  If it is missing
or an entry point fails, this module raises - it never routes to NumPy/torch.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# $XV_LIB: an alternative build of the same C-ABI (tools/variant.sh builds, tools/ab.sh / tools/probe.sh compare them on the GPU box); never a different backend
LIB_PATH = os.environ.get("XV_LIB") or os.path.join(_HERE, "libxvector_hip.so")

c_float_p = C.POINTER(C.c_float)
c_int32_p = C.POINTER(C.c_int32)


class XvError(RuntimeError):
    pass


# include/xvector_hip.h XV_ABI_VERSION: the layout of XvConfig below and the SIGNATURES table belong to this version
ABI_VERSION = 3


class _SizedConfig(C.Structure):
    """Base of the mirrors of the header's config structures: keyword arguments only, on top of DEFAULTS; struct_bytes is filled in here."""
    DEFAULTS = {}

    def __init__(self, *args, **kw):
        if args:      # struct_bytes is the first field: a positional XvConfig(feat_dim, ...) would shift every value by one, silently
            raise TypeError("%s takes keyword arguments only (its first field is struct_bytes, filled in here)" % type(self).__name__)
        super(_SizedConfig, self).__init__(**dict(self.DEFAULTS, **kw))
        self.struct_bytes = C.sizeof(type(self))


class XvConfig(_SizedConfig):
    """Mirror of `struct xv_config` (include/xvector_hip.h); no defaults: engine.make_config states every field it relies on."""

    _fields_ = [
        ("struct_bytes", C.c_int32),
        ("feat_dim", C.c_int32),
        ("num_speakers", C.c_int32),
        ("num_nodes_pooling_layer", C.c_int32),
        ("num_nodes_last_layer", C.c_int32),
        ("last_layer_no_bn", C.c_int32),
        ("last_layer_linear", C.c_int32),
        ("feature_norm", C.c_int32),
        ("feature_scaling_factor", C.c_float),
        ("loss_kind", C.c_int32),
        ("margin_m", C.c_float),
        ("lambda_min", C.c_float),
        ("lambda_base", C.c_float),
        ("lambda_gamma", C.c_float),
        ("lambda_power", C.c_float),
        ("weight_l2_regularizer", C.c_float),
        ("output_weight_l2_regularizer", C.c_float),
        ("batchnorm_momentum", C.c_float),
        ("bn_epsilon", C.c_float),
        ("fused_bn_unbiased_moving_var", C.c_int32),
        ("optimizer", C.c_int32),
        ("momentum", C.c_float),
        ("use_nesterov", C.c_int32),
        ("clip_gradient_norm", C.c_float),
        ("max_batch", C.c_int32),
        ("max_frames", C.c_int32),
        ("precision", C.c_int32),
        ("pooling", C.c_int32),
        ("att_key0_nodes", C.c_int32),
        ("att_key1_nodes", C.c_int32),
        ("att_key_type", C.c_int32),
        ("att_use_scale", C.c_int32),
        ("aux_ring", C.c_int32),
        ("ring_loss_init", C.c_float),
        ("ring_loss_lambda", C.c_float),
        ("aux_mhe", C.c_int32),
        ("mhe_lambda", C.c_float),
        ("num_frame_layers", C.c_int32),
        ("frame_context", C.c_int32 * 12),
        ("frame_width", C.c_int32 * 12),
        ("relu_type", C.c_int32),
        ("max_rows", C.c_int32),
        ("vlad_num_centers", C.c_int32),
        ("vlad_num_ghosts", C.c_int32),
        ("vlad_final_l2_norm", C.c_int32),
    ]


class XvMfccConfig(_SizedConfig):
    """Mirror of `struct xv_mfcc_config` (include/xvector_hip.h) with its defaults - the VoxCeleb conf/mfcc.conf, dither 0."""

    _fields_ = [
        ("struct_bytes", C.c_int32),
        ("sample_frequency", C.c_float),
        ("frame_length_ms", C.c_float),
        ("frame_shift_ms", C.c_float),
        ("num_mel_bins", C.c_int32),
        ("num_ceps", C.c_int32),
        ("low_freq", C.c_float),
        ("high_freq", C.c_float),
        ("snip_edges", C.c_int32),
        ("preemphasis", C.c_float),
        ("remove_dc_offset", C.c_int32),
        ("cepstral_lifter", C.c_float),
        ("use_energy", C.c_int32),
        ("raw_energy", C.c_int32),
        ("energy_floor", C.c_float),
    ]
    DEFAULTS = dict(sample_frequency=16000.0, frame_length_ms=25.0, frame_shift_ms=10.0, num_mel_bins=30, num_ceps=30, low_freq=20.0,
                    high_freq=7600.0, snip_edges=0, preemphasis=0.97, remove_dc_offset=1, cepstral_lifter=22.0, use_energy=1, raw_energy=1,
                    energy_floor=0.0)


class XvFbankConfig(_SizedConfig):
    """Mirror of `struct xv_fbank_config` (include/xvector_hip.h) with its defaults - compute-fbank-feats' own, dither 0."""

    _fields_ = [
        ("struct_bytes", C.c_int32),
        ("sample_frequency", C.c_float),
        ("frame_length_ms", C.c_float),
        ("frame_shift_ms", C.c_float),
        ("num_mel_bins", C.c_int32),
        ("low_freq", C.c_float),
        ("high_freq", C.c_float),
        ("snip_edges", C.c_int32),
        ("preemphasis", C.c_float),
        ("remove_dc_offset", C.c_int32),
        ("use_energy", C.c_int32),
        ("raw_energy", C.c_int32),
        ("energy_floor", C.c_float),
        ("use_log_fbank", C.c_int32),
        ("use_power", C.c_int32),
    ]
    DEFAULTS = dict(sample_frequency=16000.0, frame_length_ms=25.0, frame_shift_ms=10.0, num_mel_bins=23, low_freq=20.0, high_freq=0.0,
                    snip_edges=1, preemphasis=0.97, remove_dc_offset=1, use_energy=0, raw_energy=1, energy_floor=0.0, use_log_fbank=1,
                    use_power=1)


class XvAugmentConfig(_SizedConfig):
    """Mirror of `struct xv_augment_config` (include/xvector_hip.h) with its defaults - wav-reverberate --shift-output=true
    --normalize-output=true at 16 kHz."""

    _fields_ = [
        ("struct_bytes", C.c_int32),
        ("sample_frequency", C.c_float),
        ("shift_output", C.c_int32),
        ("normalize_output", C.c_int32),
        ("volume", C.c_float),
    ]
    DEFAULTS = dict(sample_frequency=16000.0, shift_output=1, normalize_output=1, volume=0.0)


class XvResampleConfig(_SizedConfig):
    """Mirror of `struct xv_resample_config` (include/xvector_hip.h): fin and fout must be given; zeros mean the defaults (6 zeros, the
    cutoff 0.99 * 0.5 * min(fin, fout))."""

    _fields_ = [
        ("struct_bytes", C.c_int32),
        ("fin", C.c_int32),
        ("fout", C.c_int32),
        ("num_zeros", C.c_int32),
        ("cutoff", C.c_float),
    ]
    DEFAULTS = dict(fin=0, fout=0, num_zeros=0, cutoff=0.0)


class XvPairLossConfig(_SizedConfig):
    """Mirror of `struct xv_pair_loss_config` (include/xvector_hip.h): the options of the pairwise loss heads; the defaults are the semi-hard
    loss, unsquared, margin 0."""

    _fields_ = [
        ("struct_bytes", C.c_int32),
        ("kind", C.c_int32),
        ("squared", C.c_int32),
        ("triplet_type", C.c_int32),
        ("margin_kind", C.c_int32),
        ("margin", C.c_float),
        ("valid_speakers", C.c_int32),
        ("valid_segments", C.c_int32),
    ]
    DEFAULTS = dict(kind=0, squared=0, triplet_type=0, margin_kind=2, margin=0.0, valid_speakers=0, valid_segments=0)


class XvGe2eConfig(_SizedConfig):
    """Mirror of `struct xv_ge2e_config` (include/xvector_hip.h): the options of the GE2E training loss; the defaults are the softmax type
    on an unset layout (the entry points refuse 0 speakers)."""

    _fields_ = [
        ("struct_bytes", C.c_int32),
        ("loss_type", C.c_int32),
        ("speakers", C.c_int32),
        ("segments", C.c_int32),
        ("valid_speakers", C.c_int32),
        ("valid_segments", C.c_int32),
    ]
    DEFAULTS = dict(loss_type=0, speakers=0, segments=0, valid_speakers=0, valid_segments=0)


GE2E_TYPES = {"softmax": 0, "contrastive": 1}                             # XV_GE2E_SOFTMAX / XV_GE2E_CONTRASTIVE
PAIR_KINDS = {"semihard_triplet_loss": 0, "angular_triplet_loss": 1}      # XV_PAIR_SEMIHARD / XV_PAIR_ANGULAR
TRIPLET_TYPES = {"all": 0, "hard": 1}                                     # XV_TRIPLET_ALL / XV_TRIPLET_HARD
LOSS_KINDS = {
    "softmax": 0,
    "asoftmax": 1,
    "additive_margin_softmax": 2,
    "additive_angular_margin_softmax": 3,
    "semihard_triplet_loss": 4,          # XV_LOSS_SEMIHARD_TRIPLET / XV_LOSS_ANGULAR_TRIPLET: the pairwise heads (XvPairLossConfig carries their options)
    "angular_triplet_loss": 5,
    "ge2e_loss": 6,                      # XV_LOSS_GE2E: the GE2E training loss (XvGe2eConfig carries its options)
}
OPTIMIZERS = {"sgd": 0, "momentum": 1, "adam": 2}
PRECISIONS = {"f32": 0, "f16x3": 1}
POOLINGS = {"statistics_pooling": 0, "self_attention": 1, "ghost_vlad": 2}
RELU_TYPES = {"relu": 0, "prelu": 1, "lrelu": 2}

_VP = C.c_void_p
_SZ = C.c_size_t
_I = C.c_int
_F = C.c_float

# name -> (restype, argtypes).  Kept in header order; tests/test_abi.py checks every entry against the prototype of
# include/xvector_hip.h, type by type, and that the .so exports it.
SIGNATURES = {
    "xv_last_error": (C.c_char_p, []),
    "xv_abi_version": (_I, []),
    "xv_device_count": (_I, []),
    "xv_profile_begin": (_I, [_I]),
    "xv_profile_begin_kinds": (_I, [_I, C.c_uint32]),
    "xv_profile_end": (_I, [C.POINTER(C.c_int64), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "xv_debug_nt_schedule": (_I, [_I, _I, _I, _I, _I]),
    "xv_debug_tn_plan": (_I, [_I, _I, _I, _I, C.POINTER(_I)]),
    "xv_debug_softmax_rows_form": (_I, [_I, C.c_size_t, C.c_size_t]),
    "xv_debug_col_stats_form": (_I, [_I, _I, C.c_size_t, C.c_size_t]),
    "xv_debug_bn_bwd_plan": (_I, [_I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, C.POINTER(_I)]),
    "xv_debug_segment_plan": (_I, [_I, _I, _I, _SZ, C.POINTER(_I)]),
    "xv_debug_att_score_form": (_I, [_I, _I, C.c_size_t, C.c_size_t]),
    "xv_debug_gemm16_nt_form": (_I, [_I, _I, _I, _I, _I, _I, _I, _I, _I, C.POINTER(_I)]),
    "xv_debug_gemm16_tn_plan": (_I, [_I, _I, _I, _I, _I, _I, C.POINTER(_I)]),
    "xv_debug_engine_clip_sumsq": (_I, [_VP, C.POINTER(_VP)]),
    "xv_copy_2d": (_I, [_VP, _VP, _SZ, _VP, _SZ, _I, _I]),
    "xv_op_workspace_bytes": (_SZ, [_I, _I, _I]),
    "xv_pad_channels": (_I, [_VP, _VP, _I, _I, _VP, _I]),
    "xv_prep_weight_fwd": (_I, [_VP, _VP, _I, _I, _I, _VP, _I]),
    "xv_prep_weight_dgrad": (_I, [_VP, _VP, _I, _I, _I, _VP]),
    "xv_affine_forward": (_I, [_VP, _VP, _I, _I, _I, _I, _VP, _VP, _VP, _I, _I, _VP, _VP, _SZ]),
    "xv_affine_dgrad": (_I, [_VP, _VP, _I, _I, _I, _I, _VP, _VP, _I, _VP, _SZ]),
    "xv_affine_wgrad": (_I, [_VP, _VP, _I, _I, _I, _I, _I, _VP, _I, _I, _I, _VP, _F, _VP, _VP, _SZ]),
    "xv_colsum": (_I, [_VP, _VP, _I, _I, _I, _VP, _VP, _SZ]),
    "xv_col_stats": (_I, [_VP, _VP, _I, _I, _I, _VP]),
    "xv_bn_finalize": (_I, [_VP, _VP, _I, _I, _VP, _VP, _F, _F, _I, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _I]),
    "xv_bn_inference_scale": (_I, [_VP, _I, _VP, _VP, _VP, _VP, _F, _VP, _VP]),
    "xv_bn_apply": (_I, [_VP, _VP, _I, _I, _I, _VP, _VP, _I, _VP, _I]),
    "xv_bn_relu_backward": (_I, [_VP, _VP, _VP, _I, _I, _I, _VP, _VP, _VP, _VP, _VP, _I, _I, _VP, _VP, _VP, _VP, _VP, _SZ]),
    "xv_prelu_forward": (_I, [_VP, _VP, _I, _I, _VP, _VP]),
    "xv_set_activation": (_I, [_VP, _VP]),
    "xv_relu_backward": (_I, [_VP, _VP, _VP, _SZ, _VP]),
    "xv_amax": (_I, [_VP, _VP, _SZ, _VP]),
    "xv_split_planes": (_I, [_VP, _VP, _I, _I, _I, _VP, _I, _SZ, _VP]),
    "xv_bn_apply_split": (_I, [_VP, _VP, _I, _I, _I, _VP, _VP, _I, _VP, _VP, _I, _SZ]),
    "xv_bn_output_range": (_I, [_VP, _VP, _I, _I, _VP, _VP, _I, _VP, _VP, _VP]),
    "xv_bn_relu_backward_split": (_I, [_VP, _VP, _VP, _I, _I, _I, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _I, _I, _VP, _I, _SZ, _VP, _VP, _VP,
                                       _VP, _VP, _SZ]),
    "xv_affine_forward_f16x3": (_I, [_VP, _VP, _SZ, _VP, _I, _I, _I, _I, _VP, _SZ, _VP, _VP, _VP, _I, _I, _VP]),
    "xv_affine_dgrad_f16x3": (_I, [_VP, _VP, _SZ, _VP, _I, _I, _I, _I, _VP, _SZ, _VP, _VP, _I]),
    "xv_affine_dgrad_bnstats_f16x3": (_I, [_VP, _VP, _SZ, _VP, _I, _I, _I, _I, _VP, _SZ, _VP, _VP, _I, _VP, _VP, _VP, _VP, _VP, _VP]),
    "xv_bn_relu_backward_split_from_part": (_I, [_VP, _VP, _I, _VP, _VP, _I, _I, _I, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _I, _VP, _I, _SZ,
                                                 _VP, _VP, _VP, _VP, _VP, _SZ]),
    "xv_affine_wgrad_f16x3": (_I, [_VP, _VP, _SZ, _VP, _I, _I, _I, _I, _I, _VP, _SZ, _VP, _I, _I, _I, _I, _VP, _F, _VP, _VP, _SZ]),
    "xv_stat_pool_forward": (_I, [_VP, _VP, _I, _I, _I, _VP]),
    "xv_stat_pool_backward": (_I, [_VP, _VP, _VP, _VP, _I, _I, _I, _VP]),
    "xv_stat_pool_forward_bn": (_I, [_VP, _VP, _I, _I, _I, _VP, _VP, _I, _VP, _VP]),
    "xv_bn_relu_backward_pooled": (_I, [_VP, _VP, _VP, _VP, _I, _I, _VP, _I, _VP, _VP, _VP, _VP, _VP, _I, _VP, _VP, _VP, _VP, _VP, _SZ]),
    "xv_stat_pool_forward_bn_aux": (_I, [_VP, _VP, _I, _I, _I, _VP, _VP, _I, _VP, _VP, _VP, _VP]),
    "xv_bn_relu_backward_pooled_aux": (_I, [_VP, _VP, _VP, _VP, _VP, _I, _I, _VP, _I, _VP, _VP, _VP, _VP, _VP, _I, _VP, _VP, _VP, _VP, _VP, _SZ]),
    "xv_bn_relu_backward_pooled_split": (_I, [_VP, _VP, _VP, _VP, _I, _I, _VP, _I, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _I, _VP, _I, _SZ, _VP,
                                              _VP, _VP, _VP, _VP, _SZ]),
    "xv_ring_loss": (_I, [_VP, _VP, _I, _I, _I, _VP, _F, _VP, _VP, _VP]),
    "xv_mhe_loss": (_I, [_VP, _VP, _I, _I, _I, _VP, _I, _F, _VP, _VP, _VP]),
    "xv_mhe_add_grad": (_I, [_VP, _VP, _I, _I, _I, _VP, _VP]),
    "xv_att_score": (_I, [_VP, _VP, _I, _I, _I, _I, _VP, _F, _VP]),
    "xv_softmax_segments": (_I, [_VP, _VP, _I, _I, _VP]),
    "xv_softmax_segments_backward": (_I, [_VP, _VP, _VP, _I, _I, _VP]),
    "xv_att_pool_backward_weights": (_I, [_VP, _VP, _I, _I, _I, _VP, _VP, _I, _VP, _VP, _VP]),
    "xv_att_key_backward": (_I, [_VP, _VP, _I, _I, _I, _VP, _F, _VP, _VP, _VP, _VP, _VP, _SZ]),
    "xv_key_activation": (_I, [_VP, _VP, _SZ, _I, _VP]),
    "xv_add_inplace": (_I, [_VP, _VP, _VP, _SZ]),
    "xv_vlad_softmax": (_I, [_VP, _VP, _I, _I, _I, _VP]),
    "xv_vlad_repitch": (_I, [_VP, _VP, _I, _I, _I, _VP, _I]),
    "xv_vlad_pool_forward": (_I, [_VP, _VP, _VP, _VP, _I, _I, _I, _I, _I, _VP, _I, _VP, _VP]),
    "xv_vlad_normalize_forward": (_I, [_VP, _VP, _I, _I, _I, _I, _VP]),
    "xv_vlad_normalize_backward": (_I, [_VP, _VP, _VP, _I, _I, _I, _I, _VP]),
    "xv_vlad_pool_backward": (_I, [_VP, _VP, _VP, _VP, _VP, _I, _I, _I, _I, _I, _VP, _VP]),
    "xv_vlad_softmax_backward": (_I, [_VP, _VP, _VP, _I, _I, _I, _VP]),
    "xv_vlad_centers_backward": (_I, [_VP, _VP, _VP, _VP, _I, _I, _I, _I, _F, _VP]),
    "xv_l2_scaling_forward": (_I, [_VP, _VP, _I, _I, _F, _VP]),
    "xv_l2_scaling_backward": (_I, [_VP, _VP, _VP, _I, _I, _F, _VP]),
    "xv_loss_prep_weight": (_I, [_VP, _VP, _I, _I, _I, _VP, _VP, _I, _VP]),
    "xv_margin_softmax_rows": (_I, [_VP, _I, _VP, _I, _I, _I, _VP, _I, _VP, _F, _F, _VP, _VP, _VP, _VP]),
    "xv_cm_decode": (_I, [_VP, _VP, _I, _I, _I, _SZ, _VP]),
    "xv_cm_decode_ragged": (_I, [_VP, _VP, _VP, _VP, _I, _I, _I, _VP]),
    "xv_cm_encode": (_I, [_VP, _VP, _VP, _I, _I, _I, _I, _VP, _VP]),
    "xv_frontend": (_I, [_VP, _VP, _VP, _I, _I, _I, _I, _VP, _SZ, _VP, _VP, _VP, _I, _VP, _VP, _VP, _SZ]),
    "xv_mfcc_num_frames": (C.c_int64, [_VP, C.c_int64]),
    "xv_mfcc_table_floats": (_SZ, [_VP]),
    "xv_mfcc_tables": (_I, [_VP, _VP, _SZ]),
    "xv_mfcc": (_I, [_VP, _VP, _VP, _VP, _VP, _VP, _I, _I, _VP, _VP]),
    "xv_energy_vad": (_I, [_VP, _VP, _VP, _I, _I, _I, _F, _F, _I, _F, _VP]),
    "xv_fbank_num_frames": (C.c_int64, [_VP, C.c_int64]),
    "xv_fbank_table_floats": (_SZ, [_VP]),
    "xv_fbank_tables": (_I, [_VP, _VP, _SZ]),
    "xv_fbank": (_I, [_VP, _VP, _VP, _VP, _VP, _VP, _I, _I, _VP, _VP, _VP]),
    "xv_debug_augment_plan": (_I, [C.c_int64, C.c_int64, C.POINTER(_I)]),
    "xv_augment_workspace_bytes": (_SZ, [_I, _I, C.c_int64]),
    "xv_augment": (_I, [_VP, _VP, _I, _I, C.c_int64, _VP, _VP, _VP, _VP, _SZ, _I, _VP, _SZ, _VP, _VP, _VP, _VP]),
    "xv_resample_num_samples": (C.c_int64, [_VP, C.c_int64]),
    "xv_resample_table_floats": (_SZ, [_VP]),
    "xv_resample_tables": (_I, [_VP, _VP, _SZ]),
    "xv_debug_resample_plan": (_I, [_VP, C.POINTER(_I)]),
    "xv_resample": (_I, [_VP, _VP, _VP, _VP, _VP, _VP, _I, _VP, _VP, _VP, _VP, _VP]),
    "xv_score_prepare": (_I, [_VP, _VP, _I, _I, _I, _VP, _VP, _I]),
    "xv_score_trials": (_I, [_VP, _VP, _I, _I, _VP, _I, _I, _I, _VP, _VP, C.c_int64, _VP, _VP, _VP]),
    "xv_score_cohort_workspace_bytes": (_SZ, [_I, _I, _I]),
    "xv_score_cohort_stats": (_I, [_VP, _VP, _I, _I, _VP, _I, _I, _I, _I, _VP, _VP, _SZ]),
    "xv_score_normalize": (_I, [_VP, _VP, _VP, _VP, C.c_int64, _VP, _VP, _VP]),
    "xv_score_dense": (_I, [_VP, _VP, _I, _I, _I, _VP, _I]),
    "xv_backend_group_means": (_I, [_VP, _VP, _I, _I, _I, _VP, _VP, _I, C.c_int64, _VP, _VP, _I]),
    "xv_backend_center": (_I, [_VP, _VP, _I, _I, _I, _VP, _VP, _I]),
    "xv_backend_scatter_workspace_bytes": (_SZ, [_I, _I]),
    "xv_backend_scatter": (_I, [_VP, _VP, _I, _I, _I, _VP, _VP, _VP, _SZ]),
    "xv_backend_plda_normalize": (_I, [_VP, _VP, _I, _I, _I, _VP, _VP, _VP, _I]),
    "xv_backend_plda_trials": (_I, [_VP, _VP, _I, _I, _VP, _I, _I, _I, _VP, _VP, C.c_int64, _VP, _VP, _I, _I, _VP, _VP, _VP]),
    "xv_backend_plda_cohort_workspace_bytes": (_SZ, [_I, _I, _I, _I]),
    "xv_backend_plda_cohort_stats": (_I, [_VP, _VP, _I, _I, _VP, _VP, _I, _I, _I, _VP, _I, _I, _VP, _VP, _I, _VP, _VP, _SZ]),
    "xv_backend_plda_dense_workspace_bytes": (_SZ, [_I, _I]),
    "xv_backend_plda_dense": (_I, [_VP, _VP, _I, _I, _I, _VP, _I, _VP, _VP, _VP, _I, _VP, _SZ]),
    "xv_backend_pca_plda_workspace_bytes": (_SZ, [_I, _I]),
    "xv_backend_pca_plda": (_I, [_VP, _VP, C.c_int64, _VP, _VP, _VP, _I, _I, _I, C.c_double, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP,
                                 _VP, _VP, _VP, _SZ]),
    "xv_ahc_workspace_bytes": (_SZ, [C.c_int64]),
    "xv_ahc_cluster": (_I, [_VP, _VP, C.c_int64, _VP, _VP, _VP, _VP, _I, _I, C.c_int64, C.c_int64, _F, _VP, _VP, _VP, _VP, _VP, _SZ]),
    "xv_ahc_cluster_from_workspace_bytes": (_SZ, [C.c_int64]),
    "xv_ahc_cluster_from": (_I, [_VP, _VP, C.c_int64, _VP, _VP, _VP, _VP, _VP, _I, _I, _I, C.c_int64, C.c_int64, _F, _VP, _VP, _VP, _VP, _VP, _SZ]),
    "xv_ahc_cluster_sums_workspace_bytes": (_SZ, [_I, C.c_int64]),
    "xv_ahc_cluster_sums": (_I, [_VP, _VP, C.c_int64, _VP, _VP, _VP, _VP, _VP, _VP, _I, _I, _I, C.c_int64, C.c_int64, C.c_int64, C.c_int64, _VP, _VP,
                                 _VP, _VP, _SZ]),
    "xv_ahc_cut": (_I, [_VP, _VP, _VP, _VP, _VP, _I, _I, C.c_int64, _VP, _VP, _VP, _I, _VP, _VP]),
    "xv_diar_confusion": (_I, [_VP, _VP, _VP, _VP, _VP, _VP, _VP, _I, C.c_int64, C.c_int64, _VP, _VP, _VP, _I, C.c_int64, _VP, _VP, _VP]),
    "xv_vbx_workspace_bytes": (_SZ, [C.c_int64, C.c_int64, C.c_int64, _I]),
    "xv_vbx": (_I, [_VP, _VP, C.c_int64, _VP, _VP, _VP, _VP, _I, _I, _I, _I, C.c_int64, C.c_int64, C.c_int64, _VP, _VP, _VP, _F, _F, _F, _I, C.c_double,
                    _VP, _VP, _VP, _VP, _VP, _VP, _SZ]),
    "xv_add_norm_grad": (_I, [_VP, _VP, _VP, _I, _I, _VP]),
    "xv_segment_gemm": (_I, [_VP, _VP, C.c_long, _VP, C.c_long, _I, _I, _I, _VP, _VP, _VP, _VP, C.c_long, _VP, C.c_long, _VP, _SZ, _VP]),
    "xv_segment_affine_bn_forward": (_I, [_VP, _VP, C.c_long, _VP, C.c_long, _I, _I, _I, _VP, _VP, _VP, _F, _F, _I, _VP, _VP, _VP, _VP, _VP,
                                          _VP, _VP, _I, _VP, _VP, _SZ, _VP]),
    "xv_segment_dgrad_bn_backward": (_I, [_VP, _VP, C.c_long, _VP, C.c_long, _I, _I, _I, _VP, _VP, _VP, C.c_long, _VP, _VP, _VP, _VP, _VP,
                                          _VP, _I, _VP, _VP, _VP, _VP, _VP, _SZ, _VP]),
    "xv_pair_loss_workspace_bytes": (_SZ, [_I, _I]),
    "xv_pair_loss_forward": (_I, [_VP, C.POINTER(XvPairLossConfig), _VP, _I, _I, _I, _VP, _VP, _VP, _VP, _SZ]),
    "xv_pair_loss_backward": (_I, [_VP, C.POINTER(XvPairLossConfig), _VP, _I, _I, _I, _VP, _VP, _SZ, _VP, _I]),
    "xv_e2e_valid_loss": (_I, [_VP, _VP, _I, _I, _I, _I, _VP, _VP, _SZ]),
    "xv_ge2e_loss_workspace_bytes": (_SZ, [_I, _I, _I]),
    "xv_ge2e_loss_forward": (_I, [_VP, C.POINTER(XvGe2eConfig), _VP, _I, _I, _VP, _VP, _VP, _VP, _VP, _SZ]),
    "xv_ge2e_loss_backward": (_I, [_VP, C.POINTER(XvGe2eConfig), _VP, _I, _I, _VP, _VP, _VP, _SZ, _VP, _I, _VP, _VP]),
    "xv_loss_weight_backward": (_I, [_VP, _VP, _I, _VP, _I, _VP, _VP, _I, _I, _I, _F, _VP, _VP, _SZ]),
    "xv_l2_reg_loss": (_I, [_VP, _VP, _SZ, _F, _VP]),
    "xv_sgd_update": (_I, [_VP, _VP, _VP, _SZ, _F, _F]),
    "xv_momentum_update": (_I, [_VP, _VP, _VP, _VP, _SZ, _F, _F, _I, _F]),
    "xv_adam_update": (_I, [_VP, _VP, _VP, _VP, _VP, _SZ, _F, _F, _F, _F, _I, _F]),
    "xv_sumsq": (_I, [_VP, _VP, _SZ, _VP]),
    "xv_engine_create": (_I, [C.POINTER(XvConfig), C.POINTER(_VP)]),
    "xv_engine_destroy": (None, [_VP]),
    "xv_engine_num_variables": (_I, [_VP]),
    "xv_engine_variable_info": (_I, [_VP, _I, C.POINTER(C.c_char_p), c_int32_p, c_int32_p, C.POINTER(_SZ), c_int32_p]),
    "xv_engine_variables_count": (_SZ, [_VP]),
    "xv_engine_trainable_count": (_SZ, [_VP]),
    "xv_engine_optimizer_state_count": (_SZ, [_VP]),
    "xv_engine_bind": (_I, [_VP, _VP, _VP, _VP]),
    "xv_engine_forward": (_I, [_VP, _VP, _VP, _I, _I, _I]),
    "xv_engine_forward_lengths": (_I, [_VP, _VP, _VP, _I, _I, _VP]),
    "xv_engine_loss_forward": (_I, [_VP, _VP, _VP, _I, _I]),
    "xv_engine_set_pair_loss": (_I, [_VP, C.POINTER(XvPairLossConfig)]),
    "xv_engine_set_ge2e_loss": (_I, [_VP, C.POINTER(XvGe2eConfig)]),
    "xv_engine_backward": (_I, [_VP, _VP, _I]),
    "xv_engine_backward_async": (_I, [_VP, _VP, _I]),
    "xv_engine_stage_wait": (_I, [_VP, _VP, _I]),
    "xv_engine_allreduce": (_I, [_VP, _VP, _I, _VP]),
    "xv_engine_allreduce_wait": (_I, [_VP, _VP]),
    "xv_engine_stage_grad_range": (_I, [_VP, _I, C.POINTER(_SZ), C.POINTER(_SZ)]),
    "xv_engine_apply": (_I, [_VP, _VP, _F, _F, _I]),
    "xv_engine_arena_bytes": (_SZ, [_VP]),
    "xv_engine_loss_ptrs": (_I, [_VP, C.POINTER(_VP), C.POINTER(_VP)]),
    "xv_engine_endpoint": (_I, [_VP, C.c_char_p, C.POINTER(_VP), c_int32_p, c_int32_p, c_int32_p]),
    "xv_engine_set_concurrency": (_I, [_VP, _I]),
    "xv_engine_invalidate_weights": (_I, [_VP]),
}

XV_AUG_UTT_WORDS = 10       # include/xvector_hip.h: words per utterance / per noise entry of xv_augment's tables
XV_AUG_NOISE_WORDS = 5
XV_CM_HEADERS = {"quartiles": 0, "uniform": 1}      # XV_CM_HEADER_QUARTILES / XV_CM_HEADER_UNIFORM
# The caps of the diarization kernels, as their units define them (tests/test_diar_ops_host.py holds each against the entry point's own
# refusal); diar_ops.py, misc/diarization.py and the diarize.py driver read them here, where no device library is loaded.
AHC_MAX_N = 2048            # csrc/xv_ahc.hip AHC_MAX_N: the rows of one recording a clusterer takes; the clusters a seeded start takes
AHC_MAX_POINTS = 32768      # ... AHC_MAX_POINTS: the rows of one recording xv_ahc_cluster_sums takes; the sizes of a seed together
DIAR_MAX_SPEAKERS = 32      # csrc/xv_diar_eval.hip DE_MAX_SPEAKERS: the reference speakers of one recording xv_diar_confusion takes (a bit each)
DIAR_MAX_CLUSTERS = 256     # ... DE_MAX_CLUSTERS: the hypothesis clusters of one (recording, cut) it counts
VBX_MAX_ROWS = 2048         # csrc/xv_vbx.hip VBX_MAX_T: the rows of one recording xv_vbx takes
VBX_MAX_SPEAKERS = 32       # ... VBX_MAX_S: its speakers (HMM states)
VBX_MAX_DIM = 256           # ... VBX_MAX_D: the dimensions of its rows
VBX_MAX_ITERS = 64          # ... VBX_MAX_ITERS: the iterations of one call
PCA_MAX_ROWS = 2048         # csrc/xv_backend_pca.hip PCA_MAX_N: the rows of one recording xv_backend_pca_plda takes
PCA_MAX_DIM = 256           # ... PCA_MAX_D: the dimensions of its rows
XV_BWD_STAGES = 4
XV_MAX_FRAME_LAYERS = 12
_lib = None


def load():
    """Load libxvector_hip.so (built in-tree by `make -C tf_kaldi_speaker_amd/csrc`,
    or `python -c 'import __graft_entry__ as g; g.build()'`).  Raises if absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.isfile(LIB_PATH):
        raise XvError(
            "HIP extension %s is missing - build it with `make -C %s` (hipcc, gfx950). "
            "There is no CPU fallback." % (LIB_PATH, os.path.join(_HERE, "csrc")))
    # torch ships its own libamdhip64 (same SONAME as /opt/rocm's).  Whichever HIP runtime is mapped first serves the whole
    # process: if this library came first it would bind the system runtime and torch's CUDA initialisation would then find
    # "no ROCm-capable device".  Importing torch first makes both share torch's runtime (device buffers are torch's anyway).
    import torch  # noqa: F401
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)   # AttributeError here == ABI mismatch: fail loudly
        fn.restype = res
        fn.argtypes = args
    if lib.xv_abi_version() != ABI_VERSION:
        raise XvError("ABI version mismatch: %s reports %d, this package binds version %d (stale build? run `make -C %s`)"
                      % (LIB_PATH, lib.xv_abi_version(), ABI_VERSION, os.path.join(_HERE, "csrc")))
    _lib = lib
    return lib


def check(rc, what=""):
    if rc != 0:
        msg = load().xv_last_error()
        raise XvError("%s failed (rc=%d): %s" % (what or "xv call", rc, msg.decode() if msg else "?"))


def call(name, *args):
    """Call an int-returning entry point and raise XvError on failure."""
    check(getattr(load(), name)(*args), name)


def share_gpu():
    """XV_SHARE_GPU=1 (tests of the multi-rank paths on a 1-GPU box): ranks are spread round-robin over the visible devices and
    talk over gloo, which carries device tensors through the host - RCCL refuses two ranks on one device."""
    return os.environ.get("XV_SHARE_GPU") == "1"


def local_device_index():
    """HIP device of this rank: LOCAL_RANK, modulo the device count in XV_SHARE_GPU mode."""
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if share_gpu():
        import torch
        return local_rank % max(torch.cuda.device_count(), 1)
    return local_rank


def dist_backend():
    return "gloo" if share_gpu() else "nccl"

