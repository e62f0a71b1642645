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
XV_TRAIN_FM, XV_TRAIN_DM, XV_TRAIN_CM = 1, 2, 3


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


class TrainChunk(C.Structure):
    _fields_ = [("payload_off", C.c_int64), ("header_off", C.c_int64), ("kind", C.c_int32), ("cols", C.c_int32),
                ("rows", C.c_int32), ("first_row", C.c_int32), ("gmin", C.c_float), ("grange", C.c_float)]


class PlanInfo(C.Structure):
    _fields_ = [
        ("struct_size", C.c_int32), ("node_id", C.c_int32), ("batch", C.c_int32), ("frame_level", C.c_int32),
        ("in_frames", C.c_int64), ("out_rows", C.c_int64), ("out_cols", C.c_int64),
        ("workspace_bytes", C.c_int64), ("flops", C.c_int64),
    ]


class KernelTime(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("ms", C.c_float), ("launches", C.c_int32),
                ("flops", C.c_int64), ("bytes", C.c_int64)]


vp, i32, i64, f32, f64, u32, cstr, P = C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_double, C.c_uint32, C.c_char_p, C.POINTER

# Every entry point of include/xvec_hip.h, in the header's order and under its section headings: (name, return type, argument
# types).  tests/test_binding_host.py holds each entry to the header's prototype.
SIGNATURES = (
    # model, plans, forward, profiling
    ("xv_version", cstr, ()),
    ("xv_create", i32, (P(ModelDesc), i32, P(vp))),
    ("xv_set_tensor", i32, (vp, cstr, vp, P(i64), i32)),
    ("xv_finalize", i32, (vp,)),
    ("xv_set_option", i32, (vp, cstr, i32)),
    ("xv_check_overflow", i32, (vp, i32)),
    ("xv_flags_async", i32, (vp, vp, vp)),
    ("xv_flags_decode", i32, (vp,)),
    ("xv_node_id", i32, (vp, cstr)),
    ("xv_layer_two_unit", i32, (vp, cstr)),
    ("xv_node_context", i32, (vp, i32)),
    ("xv_plan_create", i32, (vp, vp, i32, i32, vp, P(vp))),
    ("xv_plan_query", i32, (vp, P(PlanInfo))),
    ("xv_plan_destroy", None, (vp,)),
    ("xv_forward", i32, (vp, vp, vp, i32, vp, i64, vp, i64, vp)),
    ("xv_profile_begin", i32, (vp, i32)),
    ("xv_profile_end", i32, (vp, P(KernelTime), i32, P(i32))),
    # feature front-end on the GPU
    ("xv_frontend_cmn_select", i32, (i32, vp, i32, i32, vp, i32, vp, i64, i32, i32, i32, vp, vp, vp)),
    # MFCC features and energy VAD on the GPU
    ("xv_mfcc_create", i32, (P(MfccOpts), i32, P(vp))),
    ("xv_mfcc_destroy", None, (vp,)),
    ("xv_mfcc_num_frames", i64, (vp, i64)),
    ("xv_mfcc_compute", i32, (vp, vp, vp, vp, i32, vp, i64, vp)),
    ("xv_vad_energy", i32, (i32, vp, i64, vp, i32, f32, f32, i32, f32, vp, vp)),
    # Fbank features on the GPU
    ("xv_fbank_create", i32, (P(FbankOpts), i32, P(vp))),
    ("xv_fbank_destroy", None, (vp,)),
    ("xv_fbank_num_frames", i64, (vp, i64)),
    ("xv_fbank_num_feats", i32, (vp,)),
    ("xv_fbank_compute", i32, (vp, vp, vp, vp, i32, vp, i64, vp, vp)),
    # post-step on the GPU
    ("xv_length_normalize", i32, (i32, vp, i64, i64, i32, i32, vp, i64, vp)),
    ("xv_speaker_mean", i32, (i32, vp, i64, i32, vp, vp, i64, vp, i64, vp)),
    # cosine scoring on the GPU
    ("xv_score_prepare", i32, (i32, vp, i64, i64, i32, vp, vp, i64, i32, i32, i32, f32, vp, i64, vp)),
    ("xv_score_matrix", i32, (i32, vp, i64, i64, vp, i64, i64, i32, vp, i64, vp)),
    ("xv_score_pairs", i32, (i32, vp, i64, i64, vp, i64, i64, i32, vp, vp, i64, vp, vp)),
    ("xv_score_histogram", i32, (i32, vp, i64, i64, vp, vp, i64, i64, vp, i32, i32, i32, vp, vp, vp)),
    # PLDA scoring on the GPU
    ("xv_plda_prepare", i32, (i32, vp, i64, i64, i32, vp, i64, i32, i32, i32, i32, vp, vp, i32, vp, vp, i64, vp, i64, vp, vp)),
    ("xv_plda_matrix", i32, (i32, vp, i64, i64, vp, vp, i64, i64, vp, i32, vp, i64, vp)),
    ("xv_plda_pairs", i32, (i32, vp, i64, i64, vp, vp, i64, i64, vp, i32, vp, vp, i64, vp, vp)),
    ("xv_plda_histogram", i32, (i32, vp, i64, i64, vp, vp, vp, i64, i64, vp, vp, i32, f64, f64, i32, vp, vp, vp)),
    # score normalisation on the GPU
    ("xv_cohort_stats_workspace", i64, (i64, i64, i32)),
    ("xv_cohort_stats", i32, (i32, vp, i64, i64, vp, vp, vp, i64, i64, vp, vp, i32, i32, vp, vp, vp, vp, i64, vp)),
    # identification on the GPU
    ("xv_score_topk_workspace", i64, (i64, i64, i32)),
    ("xv_score_topk", i32, (i32, vp, i64, i64, vp, vp, vp, i64, i64, vp, vp, i32, i32, vp, vp, i64, vp, vp, i64, vp)),
    # speaker clustering on the GPU
    ("xv_ahc_matrix_floats", i64, (i64,)),
    ("xv_ahc_workspace", i64, (i64, vp)),
    ("xv_ahc", i32, (i32, vp, vp, vp, i64, f64, vp, vp, vp, vp, vp, vp, i64, vp)),
    # per-recording PCA adaptation of a PLDA model on the GPU
    ("xv_plda_adapt_workspace", i64, (i64, i32)),
    ("xv_plda_adapt_slot_bytes", i64, (i32,)),
    ("xv_plda_adapt", i32, (i32, vp, i64, vp, i64, i32, vp, vp, vp, f64, vp, vp, vp, vp, vp, vp, i64, vp)),
    # VB-HMM resegmentation of clustered x-vectors on the GPU
    ("xv_vbx_workspace", i64, (i64, vp, vp, i32)),
    ("xv_vbx", i32, (i32, vp, i64, vp, vp, i64, i32, vp, vp, i32, vp, vp, f64, f64, f64, i32, f64, vp, vp, vp, vp, i64, vp)),
    # classifier-head validation loss on the GPU
    ("xv_loss_prepare_classes", i32, (i32, vp, i64, i32, i64, i32, vp, i64, vp)),
    ("xv_loss_workspace", i64, (i64, i64)),
    ("xv_loss_classifier", i32, (i32, vp, i64, i64, i32, vp, vp, i64, i64, vp, i32, f64, f64, vp, vp, vp, vp, vp, i64, vp)),
    # loss and gradients of the classifier heads
    ("xv_loss_grad_workspace", i64, (i64, i64, i32)),
    ("xv_loss_grad_workspace_min", i64, (i64, i64, i32)),
    ("xv_loss_classifier_grad", i32, (i32, vp, i64, i64, i32, vp, vp, i64, i64, vp, i32, f64, f64, f64, vp, vp, vp, vp, vp, i64, vp,
                                      vp, vp, i64, vp)),
    # one optimizer step on one float32 parameter tensor
    ("xv_opt_workspace", i64, (i64,)),
    ("xv_opt_step", i32, (i32, i32, i32, vp, vp, vp, vp, i64, f64, f64, f64, f64, i64, vp, i64, vp)),
    # one segment-level layer with its current weights, forward and backward
    ("xv_seg_workspace", i64, (i64, i32, i32)),
    ("xv_seg_workspace_min", i64, (i64, i32, i32)),
    ("xv_seg_forward", i32, (i32, vp, i64, i64, i32, vp, i64, i32, vp, vp, vp, vp, vp, i32, vp, i64, vp, i64, vp)),
    ("xv_seg_backward", i32, (i32, vp, i64, vp, i64, vp, i64, i64, i32, vp, i64, i32, vp, vp, vp, vp, i32, vp, i64, vp, vp, vp, vp,
                              vp, i64, vp)),
    # statistics pooling of the caller's own packed rows, forward and backward
    ("xv_stat_pool_forward", i32, (i32, vp, i64, i32, vp, i64, i64, vp, i64, vp, i64, vp)),
    ("xv_stat_pool_backward", i32, (i32, vp, i64, vp, i64, i32, vp, i64, i64, vp, i64, vp, i64, vp, i64, vp)),
    # self-attentive pooling of the caller's own packed rows, forward and backward
    ("xv_att_pool_workspace", i64, (i64, i64, i32, i32, i32, i32, i32)),
    ("xv_att_pool_workspace_min", i64, (i64, i64, i32, i32, i32, i32, i32)),
    ("xv_att_pool_forward", i32, (i32, vp, i64, i32, vp, i64, i32, vp, i64, i32, i32, i32, f32, vp, i64, i64, vp, i64, vp, i64,
                                  vp, i64, vp)),
    ("xv_att_pool_backward", i32, (i32, vp, i64, vp, i64, i32, vp, i64, i32, vp, i64, i32, i32, i32, f32, vp, i64, i64, vp, i64,
                                   vp, i64, vp, i64, vp, i64, vp, i64, vp, i64, vp, i64, vp)),
    # one frame-level layer on packed utterances with its current weights, forward and backward
    ("xv_tconv_workspace", i64, (i64, i64, i64, i32, i32, i32)),
    ("xv_tconv_workspace_min", i64, (i64, i64, i64, i32, i32, i32)),
    ("xv_tconv_forward_workspace", i64, (i64, i64)),
    ("xv_tconv_forward", i32, (i32, vp, i64, i32, i32, vp, i64, i64, i64, vp, i64, i32, vp, vp, vp, vp, vp, i32, vp, i64, vp, i64,
                               vp, i64, vp)),
    ("xv_tconv_backward", i32, (i32, vp, i64, vp, i64, i32, i32, vp, i64, i64, i64, vp, i64, vp, i64, i32, vp, vp, vp, vp, i32,
                                vp, i64, vp, vp, vp, vp, vp, i64, vp)),
    # one grid convolution of the ResNet on packed utterances, forward and backward, and the residual join of a block
    ("xv_gconv_workspace", i64, (i64, i64, i64, i32, i32, i32, i32, i32, i32, i32)),
    ("xv_gconv_workspace_min", i64, (i64, i64, i64, i32, i32, i32, i32, i32, i32, i32)),
    ("xv_gconv_forward_workspace", i64, (i64, i64, i32, i32)),
    ("xv_gconv_forward", i32, (i32, vp, i64, i32, i32, i32, i32, i32, i32, vp, i64, i64, i64, vp, i64, i32, vp, vp, vp, vp, vp, i32,
                               vp, i64, vp, i64, vp, i64, vp)),
    ("xv_gconv_backward", i32, (i32, vp, i64, vp, i64, i32, i32, i32, i32, i32, i32, vp, i64, i64, i64, vp, i64, vp, i64, i32, vp, vp,
                                vp, vp, i32, vp, i64, vp, vp, vp, vp, vp, i64, vp)),
    ("xv_add_act_forward", i32, (i32, vp, i64, vp, i64, i64, i32, i32, vp, i64, vp)),
    ("xv_add_act_backward", i32, (i32, vp, i64, vp, i64, vp, i64, i64, i32, i32, vp, i64, vp)),
    # batch norm in training mode behind the stored product z of a trained layer
    ("xv_bn_batch_workspace", i64, (i64, i32)),
    ("xv_bn_batch_workspace_min", i64, (i64, i32)),
    ("xv_bn_batch_forward", i32, (i32, vp, i64, i64, i32, vp, vp, i32, f64, i32, vp, vp, vp, i64, vp, vp, vp, i64, vp)),
    ("xv_bn_batch_backward", i32, (i32, vp, i64, vp, i64, i64, i32, vp, vp, vp, vp, i32, vp, i64, vp, vp, vp, i64, vp)),
    # metric-learning loss heads on the GPU
    ("xv_metric_loss_workspace", i64, (i64, vp, i32, i32)),
    ("xv_metric_loss_slot_bytes", i64, (i32, i32, i32)),
    ("xv_metric_loss", i32, (i32, vp, i64, vp, i64, i32, vp, i32, i32, f64, i32, i32, f64, f64, vp, vp, vp, vp, vp, vp, i64, vp)),
    ("xv_metric_loss_grad_workspace", i64, (i64, vp, i32, i32)),
    ("xv_metric_loss_grad", i32, (i32, vp, i64, vp, i64, i32, vp, i32, i32, f64, i32, i32, f64, vp, vp, vp, vp, vp, i64, vp, i64, vp)),
    # back-end training statistics on the GPU
    ("xv_gram_f64_workspace", i64, (i64, i32)),
    ("xv_gram_f64", i32, (i32, vp, i64, i64, i32, vp, vp, vp, vp, i64, vp)),
    ("xv_gram_f64_rows64", i32, (i32, vp, i64, i64, i32, vp, vp, vp, vp, i64, vp)),
    ("xv_class_mean_f64", i32, (i32, vp, i64, i64, i32, vp, vp, i64, vp, vp, i64, vp)),
    # score calibration and fusion on the GPU
    ("xv_logreg_workspace", i64, (i64, i32)),
    ("xv_logreg_stats", i32, (i32, vp, i64, i64, i32, vp, vp, f64, f64, f64, vp, i32, vp, vp, vp, i64, vp)),
    ("xv_score_fuse", i32, (i32, vp, i64, i64, i32, vp, vp, vp)),
    # reverberation and additive noise
    ("xv_reverb_tile", i32, (P(i32), P(i32))),
    ("xv_reverb_workspace", i64, (vp, i64, vp, i64, i64, i64, i64, i64)),
    ("xv_reverb", i32, (i32, vp, i64, vp, i64, vp, i64, vp, i64, vp, i64, vp, vp, i64, vp, vp, vp, vp, i64, vp)),
    # host-side ark I/O
    ("xv_ark_open", i32, (cstr, i32, P(vp))),
    ("xv_ark_open_scp", i32, (cstr, P(vp))),
    ("xv_ark_scp_count", i64, (vp,)),
    ("xv_ark_scp_shapes", i32, (vp, vp, vp, i64)),
    ("xv_ark_next_batch", i32, (vp, i64, i32, i32, vp, i64, vp, vp, i64, P(i32), P(i32))),
    ("xv_ark_pending_shape", i32, (vp, P(i32), P(i32))),
    ("xv_ark_skipped", i64, (vp,)),
    ("xv_ark_set_copy_threads", i32, (vp, i32)),
    ("xv_ark_error", cstr, (vp,)),
    ("xv_ark_close", None, (vp,)),
    ("xv_ark_format_vectors", i64, (vp, i32, vp, i32, i64, vp, i64)),
    ("xv_pack_rows", i64, (vp, vp, i32, vp, i32)),
    ("xv_crc32c", u32, (u32, vp, i64)),
    # training input: the stager and the batch former
    ("xv_train_batch_workspace", i64, (i64,)),
    ("xv_train_batch_decode", i32, (i32, vp, i64, vp, i64, i32, i32, vp, i64, vp, i64, vp)),
    ("xv_train_stage", i32, (cstr, i32, vp, i32, i32, vp, i64, vp, vp, vp, vp, i64)),
    # teardown and the error string
    ("xv_destroy", None, (vp,)),
    ("xv_last_error", cstr, (vp,)),
)
EXPORTS = [name for name, _, _ in SIGNATURES]

_lib = None


def declare(cdll):
    """Give every entry point of SIGNATURES on the loaded handle `cdll` its return and argument types.  Raises, naming them,
    if symbols are missing."""
    missing = [n for n in EXPORTS if not hasattr(cdll, n)]
    if missing:
        raise RuntimeError("libxvec_hip.so lacks symbols: %s" % ", ".join(missing))
    for name, restype, argtypes in SIGNATURES:
        fn = getattr(cdll, name)
        fn.restype = restype
        fn.argtypes = list(argtypes)
    return cdll


def load():
    """Load libxvec_hip.so once and declare the signatures.  Raises on any problem."""
    global _lib
    if _lib is None:
        if not os.path.isfile(LIB_PATH):
            raise RuntimeError(
                "HIP extension %s is missing: the x-vector path has no CPU fallback. "
                "Build it with __graft_entry__.build() (hipcc --offload-arch=gfx950)." % LIB_PATH)
        import torch  # noqa: F401  (loads torch's libamdhip64 first; see module docstring)
        _lib = declare(C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL))
    return _lib


def ptr(t):
    """Device or host address of a tensor for a pointer argument; None stays None (NULL)."""
    return None if t is None else C.c_void_p(t.data_ptr())


def stream(device):
    """torch's current stream on `device`, as the hipStream_t the entry points take."""
    import torch
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


class XvError(RuntimeError):
    def __init__(self, code, msg):
        RuntimeError.__init__(self, "xvec_hip error %d: %s" % (code, msg))
        self.code = code


def check(rc, handle=None):
    if rc < 0:
        msg = load().xv_last_error(handle)
        raise XvError(rc, msg.decode("utf-8", "replace") if msg else "")
    return rc
