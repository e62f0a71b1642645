"""ctypes binding of libxvec_hip.so (include/xvec_hip.h).  Plumbing only: every function
takes plain pointers/ints; torch is imported first so that the HIP runtime the library
binds to is the one torch already loaded (same SONAME libamdhip64.so.7), which is what
makes torch tensors' data_ptr() and stream handles valid inside the library.

There is NO fallback: if the shared library is missing or a symbol is absent, loading
raises and the product path is unusable (build with `python -c "import __graft_entry__ as g; g.build()"`).
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libxvec_hip.so")

XV_MAX_ATT_LAYERS = 4
XV_OK = 0
XV_ERR_INVALID = -1
XV_ERR_UNSUPPORTED = -2
XV_ERR_WORKSPACE = -6
XV_ERR_TOO_SHORT = -7
XV_PREC_F32 = 0
XV_PREC_BF16X3 = 1
XV_PREC_F16X3 = 2
XV_PREC_F16F6 = 3
XV_POOL_STATISTICS = 0
XV_POOL_SELF_ATTENTION = 1
XV_ACT_RELU, XV_ACT_LRELU, XV_ACT_PRELU = 0, 1, 2
XV_LOSS_SOFTMAX, XV_LOSS_ASOFTMAX, XV_LOSS_AMSOFTMAX, XV_LOSS_ARCSOFTMAX = 0, 1, 2, 3
XV_OPT_SGD, XV_OPT_MOMENTUM, XV_OPT_ADAM = 0, 1, 2
XV_SEG_ACT_NONE, XV_SEG_ACT_RELU, XV_SEG_ACT_LRELU = 0, 1, 2
XV_METRIC_SEMIHARD, XV_METRIC_ANGULAR_ALL, XV_METRIC_ANGULAR_HARD, XV_METRIC_GE2E_SOFTMAX, XV_METRIC_GE2E_CONTRASTIVE = 0, 1, 2, 3, 4
XV_LOGREG_MAX_SYSTEMS = 8
XV_LOGREG_MAX_THRESHOLDS = 8

EXPORTS = ["xv_version", "xv_create", "xv_set_tensor", "xv_finalize", "xv_set_option", "xv_check_overflow", "xv_flags_async", "xv_flags_decode", "xv_node_id", "xv_node_context", "xv_layer_two_unit",
           "xv_plan_create", "xv_plan_query", "xv_plan_destroy", "xv_forward", "xv_profile_begin", "xv_profile_end",
           "xv_destroy", "xv_last_error",
           "xv_frontend_cmn_select", "xv_mfcc_create", "xv_mfcc_destroy", "xv_mfcc_num_frames", "xv_mfcc_compute", "xv_vad_energy",
           "xv_fbank_create", "xv_fbank_destroy", "xv_fbank_num_frames", "xv_fbank_num_feats", "xv_fbank_compute",
           "xv_length_normalize", "xv_speaker_mean",
           "xv_score_prepare", "xv_score_matrix", "xv_score_pairs", "xv_score_histogram",
           "xv_plda_prepare", "xv_plda_matrix", "xv_plda_pairs", "xv_plda_histogram",
           "xv_cohort_stats_workspace", "xv_cohort_stats", "xv_score_topk_workspace", "xv_score_topk",
           "xv_ahc_matrix_floats", "xv_ahc_workspace", "xv_ahc", "xv_plda_adapt_workspace", "xv_plda_adapt_slot_bytes", "xv_plda_adapt",
           "xv_vbx_workspace", "xv_vbx",
           "xv_loss_prepare_classes", "xv_loss_workspace", "xv_loss_classifier",
           "xv_loss_grad_workspace", "xv_loss_grad_workspace_min", "xv_loss_classifier_grad", "xv_opt_workspace", "xv_opt_step",
           "xv_seg_workspace", "xv_seg_workspace_min", "xv_seg_forward", "xv_seg_backward",
           "xv_stat_pool_forward", "xv_stat_pool_backward",
           "xv_att_pool_workspace", "xv_att_pool_workspace_min", "xv_att_pool_forward", "xv_att_pool_backward",
           "xv_tconv_workspace", "xv_tconv_workspace_min", "xv_tconv_forward_workspace", "xv_tconv_forward", "xv_tconv_backward",
           "xv_bn_batch_workspace", "xv_bn_batch_workspace_min", "xv_bn_batch_forward", "xv_bn_batch_backward",
           "xv_metric_loss_workspace", "xv_metric_loss_slot_bytes", "xv_metric_loss",
           "xv_gram_f64_workspace", "xv_gram_f64", "xv_gram_f64_rows64", "xv_class_mean_f64",
           "xv_logreg_workspace", "xv_logreg_stats", "xv_score_fuse",
           "xv_reverb_tile", "xv_reverb_workspace", "xv_reverb",
           "xv_ark_open", "xv_ark_open_scp", "xv_ark_scp_count", "xv_ark_scp_shapes", "xv_ark_next_batch", "xv_ark_pending_shape", "xv_ark_skipped", "xv_ark_set_copy_threads", "xv_ark_error", "xv_ark_close", "xv_ark_format_vectors", "xv_crc32c", "xv_pack_rows"]


class ModelDesc(C.Structure):
    _fields_ = [
        ("struct_size", C.c_int32), ("network_type", C.c_int32), ("feat_dim", C.c_int32),
        ("channels", C.c_int32), ("pooling_type", C.c_int32), ("relu_type", C.c_int32),
        ("num_nodes_pooling_layer", C.c_int32), ("num_nodes_last_layer", C.c_int32),
        ("last_layer_no_bn", C.c_int32), ("last_layer_linear", C.c_int32),
        ("feature_norm", C.c_int32), ("feature_scaling_factor", C.c_float),
        ("att_key_input", C.c_int32), ("att_value_input", C.c_int32),
        ("att_num_key_layers", C.c_int32), ("att_key_num_nodes", C.c_int32 * XV_MAX_ATT_LAYERS),
        ("att_key_network_type", C.c_int32),
        ("att_num_value_layers", C.c_int32), ("att_value_num_nodes", C.c_int32 * XV_MAX_ATT_LAYERS),
        ("att_value_network_type", C.c_int32),
        ("att_apply_nonlinear", C.c_int32), ("att_use_scale", C.c_int32), ("att_num_heads", C.c_int32),
        ("att_split_value", C.c_int32), ("att_split_key", C.c_int32), ("precision", C.c_int32),
        ("resnet_blocks", C.c_int32 * 4), ("resnet_maxpooling", C.c_int32), ("resnet_time_stride", C.c_int32),
    ]


class MfccOpts(C.Structure):
    _fields_ = [
        ("struct_size", C.c_int32), ("sample_frequency", C.c_float), ("frame_length_ms", C.c_float),
        ("frame_shift_ms", C.c_float), ("preemphasis_coefficient", C.c_float), ("remove_dc_offset", C.c_int32),
        ("window_type", C.c_int32), ("round_to_power_of_two", C.c_int32), ("snip_edges", C.c_int32), ("dither", C.c_float),
        ("num_mel_bins", C.c_int32), ("low_freq", C.c_float), ("high_freq", C.c_float), ("num_ceps", C.c_int32),
        ("cepstral_lifter", C.c_float), ("use_energy", C.c_int32), ("energy_floor", C.c_float), ("raw_energy", C.c_int32),
        ("htk_compat", C.c_int32),
    ]


class FbankOpts(C.Structure):
    _fields_ = [
        ("struct_size", C.c_int32), ("sample_frequency", C.c_float), ("frame_length_ms", C.c_float),
        ("frame_shift_ms", C.c_float), ("preemphasis_coefficient", C.c_float), ("remove_dc_offset", C.c_int32),
        ("window_type", C.c_int32), ("round_to_power_of_two", C.c_int32), ("snip_edges", C.c_int32), ("dither", C.c_float),
        ("num_mel_bins", C.c_int32), ("low_freq", C.c_float), ("high_freq", C.c_float), ("use_energy", C.c_int32),
        ("energy_floor", C.c_float), ("raw_energy", C.c_int32), ("htk_compat", C.c_int32), ("use_log_fbank", C.c_int32),
        ("use_power", C.c_int32),
    ]


class ReverbUtt(C.Structure):
    _fields_ = [
        ("wave_off", C.c_int64), ("wave_len", C.c_int64), ("rir_off", C.c_int64), ("rir_len", C.c_int64),
        ("noise_begin", C.c_int64), ("noise_count", C.c_int64), ("out_off", C.c_int64), ("out_len", C.c_int64),
        ("sample_rate", C.c_double), ("duration", C.c_double), ("volume", C.c_double),
        ("shift_output", C.c_int32), ("normalize_output", C.c_int32),
    ]


class ReverbNoise(C.Structure):
    _fields_ = [("off", C.c_int64), ("len", C.c_int64), ("ext_len", C.c_int64), ("snr_db", C.c_double), ("start_time", C.c_double)]


class PlanInfo(C.Structure):
    _fields_ = [
        ("struct_size", C.c_int32), ("node_id", C.c_int32), ("batch", C.c_int32), ("frame_level", C.c_int32),
        ("in_frames", C.c_int64), ("out_rows", C.c_int64), ("out_cols", C.c_int64),
        ("workspace_bytes", C.c_int64), ("flops", C.c_int64),
    ]


class KernelTime(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("ms", C.c_float), ("launches", C.c_int32),
                ("flops", C.c_int64), ("bytes", C.c_int64)]


_lib = None


def load():
    """Load libxvec_hip.so once and declare the signatures.  Raises on any problem."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.isfile(LIB_PATH):
        raise RuntimeError(
            "HIP extension %s is missing: the x-vector path has no CPU fallback. "
            "Build it with __graft_entry__.build() (hipcc --offload-arch=gfx950)." % LIB_PATH)
    import torch  # noqa: F401  (loads torch's libamdhip64 first; see module docstring)
    lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    missing = [n for n in EXPORTS if not hasattr(lib, n)]
    if missing:
        raise RuntimeError("libxvec_hip.so lacks symbols: %s" % ", ".join(missing))
    vp, i32, i64 = C.c_void_p, C.c_int, C.c_int64
    lib.xv_version.restype = C.c_char_p
    lib.xv_version.argtypes = []
    lib.xv_last_error.restype = C.c_char_p
    lib.xv_last_error.argtypes = [vp]
    lib.xv_create.argtypes = [C.POINTER(ModelDesc), i32, C.POINTER(vp)]
    lib.xv_set_tensor.argtypes = [vp, C.c_char_p, vp, C.POINTER(i64), i32]
    lib.xv_finalize.argtypes = [vp]
    lib.xv_set_option.argtypes = [vp, C.c_char_p, i32]
    lib.xv_check_overflow.argtypes = [vp, i32]
    lib.xv_flags_async.argtypes = [vp, vp, vp]
    lib.xv_flags_decode.argtypes = [vp]
    lib.xv_node_id.argtypes = [vp, C.c_char_p]
    lib.xv_node_context.argtypes = [vp, i32]
    lib.xv_layer_two_unit.argtypes = [vp, C.c_char_p]
    lib.xv_plan_create.argtypes = [vp, vp, i32, i32, vp, C.POINTER(vp)]
    lib.xv_plan_query.argtypes = [vp, C.POINTER(PlanInfo)]
    lib.xv_plan_destroy.argtypes = [vp]
    lib.xv_plan_destroy.restype = None
    lib.xv_forward.argtypes = [vp, vp, vp, i32, vp, i64, vp, i64, vp]
    lib.xv_profile_begin.argtypes = [vp, i32]
    lib.xv_profile_end.argtypes = [vp, C.POINTER(KernelTime), i32, C.POINTER(i32)]
    lib.xv_destroy.argtypes = [vp]
    lib.xv_destroy.restype = None
    lib.xv_frontend_cmn_select.argtypes = [i32, vp, i32, i32, vp, i32, vp, i64, i32, i32, i32, vp, vp, vp]
    lib.xv_mfcc_create.argtypes = [C.POINTER(MfccOpts), i32, C.POINTER(vp)]
    lib.xv_mfcc_destroy.argtypes = [vp]
    lib.xv_mfcc_destroy.restype = None
    lib.xv_mfcc_num_frames.argtypes = [vp, i64]
    lib.xv_mfcc_num_frames.restype = i64
    lib.xv_mfcc_compute.argtypes = [vp, vp, vp, vp, i32, vp, i64, vp]
    lib.xv_vad_energy.argtypes = [i32, vp, i64, vp, i32, C.c_float, C.c_float, i32, C.c_float, vp, vp]
    lib.xv_fbank_create.argtypes = [C.POINTER(FbankOpts), i32, C.POINTER(vp)]
    lib.xv_fbank_destroy.argtypes = [vp]
    lib.xv_fbank_destroy.restype = None
    lib.xv_fbank_num_frames.argtypes = [vp, i64]
    lib.xv_fbank_num_frames.restype = i64
    lib.xv_fbank_num_feats.argtypes = [vp]
    lib.xv_fbank_compute.argtypes = [vp, vp, vp, vp, i32, vp, i64, vp, vp]
    lib.xv_length_normalize.argtypes = [i32, vp, i64, i64, i32, i32, vp, i64, vp]
    lib.xv_speaker_mean.argtypes = [i32, vp, i64, i32, vp, vp, i64, vp, i64, vp]
    lib.xv_score_prepare.argtypes = [i32, vp, i64, i64, i32, vp, vp, i64, i32, i32, i32, C.c_float, vp, i64, vp]
    lib.xv_score_matrix.argtypes = [i32, vp, i64, i64, vp, i64, i64, i32, vp, i64, vp]
    lib.xv_score_pairs.argtypes = [i32, vp, i64, i64, vp, i64, i64, i32, vp, vp, i64, vp, vp]
    lib.xv_score_histogram.argtypes = [i32, vp, i64, i64, vp, vp, i64, i64, vp, i32, i32, i32, vp, vp, vp]
    lib.xv_plda_prepare.argtypes = [i32, vp, i64, i64, i32, vp, i64, i32, i32, i32, i32, vp, vp, i32, vp, vp, i64, vp, i64, vp, vp]
    lib.xv_plda_matrix.argtypes = [i32, vp, i64, i64, vp, vp, i64, i64, vp, i32, vp, i64, vp]
    lib.xv_plda_pairs.argtypes = [i32, vp, i64, i64, vp, vp, i64, i64, vp, i32, vp, vp, i64, vp, vp]
    lib.xv_plda_histogram.argtypes = [i32, vp, i64, i64, vp, vp, vp, i64, i64, vp, vp, i32, C.c_double, C.c_double, i32, vp, vp, vp]
    lib.xv_cohort_stats_workspace.argtypes = [i64, i64, i32]
    lib.xv_cohort_stats_workspace.restype = i64
    lib.xv_cohort_stats.argtypes = [i32, vp, i64, i64, vp, vp, vp, i64, i64, vp, vp, i32, i32, vp, vp, vp, vp, i64, vp]
    lib.xv_score_topk_workspace.argtypes = [i64, i64, i32]
    lib.xv_score_topk_workspace.restype = i64
    lib.xv_score_topk.argtypes = [i32, vp, i64, i64, vp, vp, vp, i64, i64, vp, vp, i32, i32, vp, vp, i64, vp, vp, i64, vp]
    lib.xv_ahc_matrix_floats.argtypes = [i64]
    lib.xv_ahc_matrix_floats.restype = i64
    lib.xv_ahc_workspace.argtypes = [i64, vp]
    lib.xv_ahc_workspace.restype = i64
    lib.xv_ahc.argtypes = [i32, vp, vp, vp, i64, C.c_double, vp, vp, vp, vp, vp, vp, i64, vp]
    lib.xv_plda_adapt_workspace.argtypes = [i64, i32]
    lib.xv_plda_adapt_workspace.restype = i64
    lib.xv_plda_adapt_slot_bytes.argtypes = [i32]
    lib.xv_plda_adapt_slot_bytes.restype = i64
    lib.xv_plda_adapt.argtypes = [i32, vp, i64, vp, i64, i32, vp, vp, vp, C.c_double, vp, vp, vp, vp, vp, vp, i64, vp]
    lib.xv_vbx_workspace.argtypes = [i64, vp, vp, i32]
    lib.xv_vbx_workspace.restype = i64
    lib.xv_vbx.argtypes = [i32, vp, i64, vp, vp, i64, i32, vp, vp, i32, vp, vp, C.c_double, C.c_double, C.c_double, i32, C.c_double,
                           vp, vp, vp, vp, i64, vp]
    lib.xv_loss_prepare_classes.argtypes =[i32, vp, i64, i32, i64, i32, vp, i64, vp]
    lib.xv_loss_workspace.argtypes = [i64, i64]
    lib.xv_loss_workspace.restype = i64
    lib.xv_loss_classifier.argtypes = [i32, vp, i64, i64, i32, vp, vp, i64, i64, vp, i32, C.c_double, C.c_double, vp, vp, vp, vp, vp, i64, vp]
    lib.xv_loss_grad_workspace.argtypes = [i64, i64, i32]
    lib.xv_loss_grad_workspace.restype = i64
    lib.xv_loss_grad_workspace_min.argtypes = [i64, i64, i32]
    lib.xv_loss_grad_workspace_min.restype = i64
    lib.xv_loss_classifier_grad.argtypes = [i32, vp, i64, i64, i32, vp, vp, i64, i64, vp, i32, C.c_double, C.c_double, C.c_double,
                                            vp, vp, vp, vp, vp, i64, vp, vp, vp, i64, vp]
    lib.xv_opt_workspace.argtypes = [i64]
    lib.xv_opt_workspace.restype = i64
    lib.xv_opt_step.argtypes = [i32, i32, i32, vp, vp, vp, vp, i64, C.c_double, C.c_double, C.c_double, C.c_double, i64, vp, i64, vp]
    lib.xv_seg_workspace.argtypes = [i64, i32, i32]
    lib.xv_seg_workspace.restype = i64
    lib.xv_seg_workspace_min.argtypes = [i64, i32, i32]
    lib.xv_seg_workspace_min.restype = i64
    lib.xv_seg_forward.argtypes = [i32, vp, i64, i64, i32, vp, i64, i32, vp, vp, vp, vp, vp, i32, vp, i64, vp, i64, vp]
    lib.xv_seg_backward.argtypes = [i32, vp, i64, vp, i64, vp, i64, i64, i32, vp, i64, i32, vp, vp, vp, vp, i32, vp, i64, vp, vp, vp, vp,
                                    vp, i64, vp]
    lib.xv_stat_pool_forward.argtypes = [i32, vp, i64, i32, vp, i64, i64, vp, i64, vp, i64, vp]
    lib.xv_stat_pool_backward.argtypes = [i32, vp, i64, vp, i64, i32, vp, i64, i64, vp, i64, vp, i64, vp, i64, vp]
    lib.xv_att_pool_workspace.argtypes = [i64, i64, i32, i32, i32, i32, i32]
    lib.xv_att_pool_workspace.restype = i64
    lib.xv_att_pool_workspace_min.argtypes = [i64, i64, i32, i32, i32, i32, i32]
    lib.xv_att_pool_workspace_min.restype = i64
    lib.xv_att_pool_forward.argtypes = [i32, vp, i64, i32, vp, i64, i32, vp, i64, i32, i32, i32, C.c_float, vp, i64, i64, vp, i64, vp, i64,
                                        vp, i64, vp]
    lib.xv_att_pool_backward.argtypes = [i32, vp, i64, vp, i64, i32, vp, i64, i32, vp, i64, i32, i32, i32, C.c_float, vp, i64, i64, vp, i64,
                                         vp, i64, vp, i64, vp, i64, vp, i64, vp, i64, vp, i64, vp]
    lib.xv_tconv_workspace.argtypes = [i64, i64, i64, i32, i32, i32]
    lib.xv_tconv_workspace.restype = i64
    lib.xv_tconv_workspace_min.argtypes = [i64, i64, i64, i32, i32, i32]
    lib.xv_tconv_workspace_min.restype = i64
    lib.xv_tconv_forward_workspace.argtypes = [i64, i64]
    lib.xv_tconv_forward_workspace.restype = i64
    lib.xv_tconv_forward.argtypes = [i32, vp, i64, i32, i32, vp, i64, i64, i64, vp, i64, i32, vp, vp, vp, vp, vp, i32, vp, i64, vp, i64,
                                     vp, i64, vp]
    lib.xv_tconv_backward.argtypes = [i32, vp, i64, vp, i64, i32, i32, vp, i64, i64, i64, vp, i64, vp, i64, i32, vp, vp, vp, vp, i32,
                                      vp, i64, vp, vp, vp, vp, vp, i64, vp]
    lib.xv_bn_batch_workspace.argtypes = [i64, i32]
    lib.xv_bn_batch_workspace.restype = i64
    lib.xv_bn_batch_workspace_min.argtypes = [i64, i32]
    lib.xv_bn_batch_workspace_min.restype = i64
    lib.xv_bn_batch_forward.argtypes = [i32, vp, i64, i64, i32, vp, vp, i32, C.c_double, i32, vp, vp, vp, i64, vp, vp, vp, i64, vp]
    lib.xv_bn_batch_backward.argtypes = [i32, vp, i64, vp, i64, i64, i32, vp, vp, vp, vp, i32, vp, i64, vp, vp, vp, i64, vp]
    lib.xv_metric_loss_workspace.argtypes = [i64, vp, i32, i32]
    lib.xv_metric_loss_workspace.restype = i64
    lib.xv_metric_loss_slot_bytes.argtypes = [i32, i32, i32]
    lib.xv_metric_loss_slot_bytes.restype = i64
    lib.xv_metric_loss.argtypes = [i32, vp, i64, vp, i64, i32, vp, i32, i32, C.c_double, i32, i32, C.c_double, C.c_double, vp, vp, vp, vp, vp, vp, i64, vp]
    lib.xv_gram_f64_workspace.argtypes = [i64, i32]
    lib.xv_gram_f64_workspace.restype = i64
    lib.xv_gram_f64.argtypes = [i32, vp, i64, i64, i32, vp, vp, vp, vp, i64, vp]
    lib.xv_gram_f64_rows64.argtypes = [i32, vp, i64, i64, i32, vp, vp, vp, vp, i64, vp]
    lib.xv_class_mean_f64.argtypes = [i32, vp, i64, i64, i32, vp, vp, i64, vp, vp, i64, vp]
    lib.xv_logreg_workspace.argtypes = [i64, i32]
    lib.xv_logreg_workspace.restype = i64
    lib.xv_logreg_stats.argtypes = [i32, vp, i64, i64, i32, vp, vp, C.c_double, C.c_double, C.c_double, vp, i32, vp, vp, vp, i64, vp]
    lib.xv_score_fuse.argtypes = [i32, vp, i64, i64, i32, vp, vp, vp]
    lib.xv_reverb_tile.argtypes = [C.POINTER(i32), C.POINTER(i32)]
    lib.xv_reverb_workspace.argtypes = [vp, i64, vp, i64, i64, i64, i64, i64]
    lib.xv_reverb_workspace.restype = i64
    lib.xv_reverb.argtypes = [i32, vp, i64, vp, i64, vp, i64, vp, i64, vp, i64, vp, vp, i64, vp, vp, vp, vp, i64, vp]
    lib.xv_ark_open.argtypes = [C.c_char_p, i32, C.POINTER(vp)]
    lib.xv_ark_open_scp.argtypes = [C.c_char_p, C.POINTER(vp)]
    lib.xv_ark_scp_count.argtypes = [vp]
    lib.xv_ark_scp_count.restype = i64
    lib.xv_ark_scp_shapes.argtypes = [vp, vp, vp, i64]
    lib.xv_ark_next_batch.argtypes = [vp, i64, i32, i32, vp, i64, vp, vp, i64, C.POINTER(i32), C.POINTER(i32)]
    lib.xv_ark_pending_shape.argtypes = [vp, C.POINTER(i32), C.POINTER(i32)]
    lib.xv_ark_skipped.argtypes = [vp]
    lib.xv_ark_set_copy_threads.argtypes = [vp, i32]
    lib.xv_ark_skipped.restype = i64
    lib.xv_ark_error.argtypes = [vp]
    lib.xv_ark_error.restype = C.c_char_p
    lib.xv_ark_close.argtypes = [vp]
    lib.xv_ark_close.restype = None
    lib.xv_ark_format_vectors.argtypes = [vp, i32, vp, i32, i64, vp, i64]
    lib.xv_ark_format_vectors.restype = i64
    lib.xv_crc32c.argtypes = [C.c_uint32, vp, i64]
    lib.xv_pack_rows.argtypes = [vp, vp, i32, vp, i32]
    lib.xv_pack_rows.restype = i64
    lib.xv_crc32c.restype = C.c_uint32
    for n in EXPORTS:
        if n not in ("xv_version", "xv_last_error", "xv_plan_destroy", "xv_destroy", "xv_ark_skipped", "xv_ark_error",
                     "xv_ark_close", "xv_ark_format_vectors", "xv_ark_scp_count", "xv_crc32c", "xv_pack_rows", "xv_gram_f64_workspace",
                     "xv_loss_workspace", "xv_loss_grad_workspace", "xv_loss_grad_workspace_min", "xv_opt_workspace", "xv_seg_workspace", "xv_seg_workspace_min", "xv_bn_batch_workspace", "xv_bn_batch_workspace_min", "xv_metric_loss_workspace", "xv_metric_loss_slot_bytes", "xv_logreg_workspace", "xv_reverb_workspace", "xv_cohort_stats_workspace", "xv_score_topk_workspace", "xv_ahc_matrix_floats", "xv_ahc_workspace", "xv_plda_adapt_workspace", "xv_plda_adapt_slot_bytes", "xv_vbx_workspace", "xv_mfcc_destroy", "xv_mfcc_num_frames", "xv_fbank_destroy", "xv_fbank_num_frames"):
            getattr(lib, n).restype = i32
    _lib = lib
    return lib


class XvError(RuntimeError):
    def __init__(self, code, msg):
        RuntimeError.__init__(self, "xvec_hip error %d: %s" % (code, msg))
        self.code = code


def check(rc, handle=None):
    if rc < 0:
        msg = load().xv_last_error(handle)
        raise XvError(rc, msg.decode("utf-8", "replace") if msg else "")
    return rc
