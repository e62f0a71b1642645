/*
 * xvec_hip.h -- C ABI of libxvec_hip.so: the MI355X (gfx950) x-vector forward path.
 *
 * This is the drop-in boundary for the ONE hot path this repository accelerates: the
 * predict sub-graph the reference runs inside TensorFlow,
 *
 *     model/trainer.py:886-913   Trainer.predict  -> sess.run(self.embeddings, ...)
 *     model/trainer.py:325-338   Trainer.build("predict") / :379-383 predict_setup
 *     model/tdnn.py:36-181       tdnn()           (frame layers, pooling, segment layers)
 *     model/pooling.py:8-240     general_pooling / statistics_pooling / self_attention
 *     model/trainer.py:385-405   entire_network   (endpoints["output"], l2_scaling)
 *
 * The reference has no FFI for this path (TensorFlow *is* its backend), so the entry
 * points below are what a binding for it would need -- each cites the reference call it
 * stands in for.  Plain C types only: pointers, sizes, int codes.  All device pointers
 * are caller-owned (the Python host hands in torch tensors' data_ptr()); the library
 * owns only the packed weights (handle) and the batch-geometry index arrays (plan).
 *
 * Every function returns XV_OK (0) or a negative xv_status; it never throws or aborts.
 * The message for the last failure on a handle is xv_last_error(handle); for failures
 * with no handle (xv_create) pass NULL.
 *
 * Threading: a handle may be shared by threads for xv_plan_* calls; concurrent
 * xv_forward calls on one handle need distinct plans, distinct workspaces and distinct
 * streams (the error string and the profiling records are the only state xv_forward
 * writes on the handle; both are locked).  xv_forward only enqueues work on `stream` and
 * returns (no host synchronisation, no allocation: it may be captured into a hipGraph).
 * Stream order is the only ordering the library relies on: a plan's index arrays are filled
 * on the stream given to xv_plan_create and recycled by xv_plan_destroy, so create, run and
 * destroy the plans of a handle on ONE stream, or synchronise between streams yourself.
 */
#ifndef XVEC_HIP_H_
#define XVEC_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct xv_handle xv_handle;   /* one model resident on one device */
typedef struct xv_plan xv_plan;       /* one batch geometry (frame offsets) + output node */

typedef enum {
  XV_OK = 0,
  XV_ERR_INVALID = -1,        /* bad argument / shape mismatch / unknown name        */
  XV_ERR_UNSUPPORTED = -2,    /* network_type / pooling_type not implemented         */
  XV_ERR_MISSING_TENSOR = -3, /* xv_finalize: a variable of the graph was never set   */
  XV_ERR_HIP = -4,            /* a HIP runtime call failed                           */
  XV_ERR_STATE = -5,          /* call order violated (e.g. forward before finalize)  */
  XV_ERR_WORKSPACE = -6,      /* workspace / output buffer too small                 */
  XV_ERR_TOO_SHORT = -7       /* an utterance has fewer frames than the node needs   */
} xv_status;

/* network_type: model/trainer.py:100-110.  "tdnn" = model/tdnn.py:10-181, "extended_tdnn" = the
 * 10-frame-layer variant model/tdnn.py:343-591 (variable scope "etdnn", conv1d kernels [w,cin,cout]) */
enum { XV_NET_TDNN = 0, XV_NET_ETDNN = 1, XV_NET_RESNET18 = 2 };   /* resnet_18: model/resnet.py:152-351 */
/* pooling_type: model/pooling.py:14-23 */
enum { XV_POOL_STATISTICS = 0, XV_POOL_SELF_ATTENTION = 1 };
/* network_relu_type: model/tdnn.py:28-33 */
enum { XV_ACT_RELU = 0, XV_ACT_LRELU = 1, XV_ACT_PRELU = 2 };
/* arithmetic of the matrix products */
enum {
  XV_PREC_F32 = 0,     /* v_mfma_f32_32x32x2_f32: exact fp32 products, fp32 accumulate   */
  XV_PREC_BF16X3 = 1,  /* 3x v_mfma_f32_16x16x32_bf16 on hi/lo bf16 splits, fp32 accumulate
                          (~5e-6 relative per layer; meets the 1e-4 parity bar at 5x the MFMA rate; full fp32 range) */
  XV_PREC_F16X3 = 2,   /* 3x v_mfma_f32_16x16x32_f16 on hi/lo fp16 splits, fp32 accumulate: same kernels, layout and
                          rate as bf16x3 with 22 instead of 16 significand bits per operand (~3e-7 relative).  Weights
                          are pre-scaled per layer by a power of two into the fp16 range (undone in the epilogue);
                          activations / input features beyond +-65504 overflow to inf -- outputs are then non-finite and
                          the host mirror raises instead of returning them */
  XV_PREC_F16F6 = 3    /* f16x3 everywhere except the 5- / 7- / 9-tap temporal convolutions (input channels a multiple of 128)
                          and the stride-1 3x3 ResNet convolutions of >= 128 channels (multiples of 128), which compute hi*hi
                          on v_mfma_f32_16x16x32_f16 and the two cross terms on the block-scaled fp6 path
                          (v_mfma_scale_f32_16x16x128_f8f6f4, e2m3, one scale per 32 channels): 1.5 MFMA units per product
                          instead of 3, ~2e-6 relative on the x-vector (bar 1e-4).  Same range rule as f16x3. */
};

#define XV_MAX_ATT_LAYERS 4

/* Graph description: the hyper-parameters of nnet/config.json that shape the predict
 * graph (model/tdnn.py:28-33,114-116,152-154,163-164,173-174; model/pooling.py:72-88;
 * model/trainer.py:400-403). */
typedef struct {
  int32_t struct_size;              /* = sizeof(xv_model_desc), for ABI checking           */
  int32_t network_type;             /* XV_NET_*                                            */
  int32_t feat_dim;                 /* nnet/feature_dim (extract.py:54-55)                 */
  int32_t channels;                 /* 512 in the reference (model/tdnn.py:43); tests shrink */
  int32_t pooling_type;             /* XV_POOL_*                                           */
  int32_t relu_type;                /* XV_ACT_*                                            */
  int32_t num_nodes_pooling_layer;  /* default 1500                                        */
  int32_t num_nodes_last_layer;     /* default 512                                         */
  int32_t last_layer_no_bn;
  int32_t last_layer_linear;
  int32_t feature_norm;             /* endpoints["output"] = l2_scaling(output)            */
  float feature_scaling_factor;
  /* self-attention (model/pooling.py:55-240) */
  int32_t att_key_input;            /* N of endpoints["tdnn<N>_relu"]: a frame layer at full context (tdnn: 3..5, etdnn: 7..10) */
  int32_t att_value_input;
  int32_t att_num_key_layers;       /* len(att_key_num_nodes), 1..XV_MAX_ATT_LAYERS        */
  int32_t att_key_num_nodes[XV_MAX_ATT_LAYERS];
  int32_t att_key_network_type;     /* 0 affine, 1 +relu, 2 +bn+relu, 3 +tanh             */
  int32_t att_num_value_layers;     /* len(att_value_num_nodes), 0..XV_MAX_ATT_LAYERS      */
  int32_t att_value_num_nodes[XV_MAX_ATT_LAYERS];
  int32_t att_value_network_type;
  int32_t att_apply_nonlinear;
  int32_t att_use_scale;
  int32_t att_num_heads;
  int32_t att_split_value;
  int32_t att_split_key;
  int32_t precision;                /* XV_PREC_*                                           */
  int32_t resnet_blocks[4];         /* resnet_18: blocks per stage, default [2,2,2,2] (model/resnet.py:203-204);
                                       `channels` is then the width of stage 1 (64)            */
  int32_t resnet_maxpooling;        /* 3x3 stride-1 'same' max-pool behind conv0 (model/resnet.py:230-231)            */
  int32_t resnet_time_stride;       /* stride 2 along time in the first block of stages 2-4 (:187,239,244,249): utterance b
                                       has ceil(L_b / 8) frames behind stage 4 (tf 'same')        */
} xv_model_desc;

typedef struct {
  int32_t struct_size;
  int32_t node_id;
  int32_t batch;            /* B                                                           */
  int32_t frame_level;      /* 1: output is packed frames [out_rows, out_cols]; 0: [B, out_cols] */
  int64_t in_frames;        /* total input frames (frame_offsets[B])                       */
  int64_t out_rows;         /* rows of the output matrix                                   */
  int64_t out_cols;         /* width E of the chosen node                                  */
  int64_t workspace_bytes;  /* device scratch xv_forward needs (256-byte aligned base)     */
  int64_t flops;            /* algorithmic 2*M*N*K of the contractions this plan runs      */
} xv_plan_info;

/* Library / build identification ("xvec_hip <version> gfx950"). */
const char* xv_version(void);

/* Trainer.__init__ + build("predict") (model/trainer.py:87-219, 325-338): create the
 * predict graph for `desc` on HIP device `device`.  No weights yet. */
int xv_create(const xv_model_desc* desc, int device, xv_handle** out);

/* Saver.restore of one variable (model/trainer.py:277-295).  `tf_name` is the TensorFlow
 * variable name ("tdnn/tdnn1_conv/kernel", "tdnn/tdnn1_bn/moving_mean",
 * "tdnn/attention/query", ...); `host` is fp32, C-contiguous, in the variable's own
 * layout (conv kernels HWIO [1,k,cin,cout], dense kernels [in,out]). */
int xv_set_tensor(xv_handle* h, const char* tf_name, const float* host, const int64_t* shape, int rank);

/* End of restore: checks that every variable of the graph is present, derives the
 * per-channel BN scale/shift, packs the kernels into the MFMA tile layout and uploads. */
int xv_finalize(xv_handle* h);

/* Execution options, to be set before the plans they affect are created.  "pool_fusion" (default 1): statistics
 * pooling fused into the epilogue of the last frame-level layer; "tail_split" (default 1): deterministic K-split of
 * the last, nearly empty round of GEMM tiles.  Both change only the schedule (results agree to rounding); tests
 * switch them off to prove which path ran.  "att_fusion" (default 1): attention scores / weighted moments computed in
 * the epilogues of the last key layer / the value layer instead of from stored activations; "slab3" (default 1): one-tap
 * layers on the kernel with three activation-slab buffers (0: the two-buffer kernel, bit-identical results).
 * "first_walk" (default 1): a first layer of at most 5 taps over a feature dimension of at most 32 whose output feeds a
 * two-unit layer (XV_PREC_F16F6) runs on workgroups that walk the row tiles with their weights resident; 2: also when it
 * writes split-blocked or fp32 rows (every precision but f32); 0: always on the tile kernel of the other convolutions.
 * Bit-identical results in all three settings.
 * "grid_compact" (default 1): ResNet convolutions enumerate output bins only (0: every grid position, bit-identical);
 * "grid_f6" (default 1; set before xv_finalize, it decides the weight formats): XV_PREC_F16F6 runs the eligible ResNet
 * convolutions on the two-unit kernel (0: on the f16x3 kernels).
 * "profile_dominant" (default 0): xv_profile_* brackets only the step
 * with the most algorithmic FLOPs of each plan (two events per forward instead of two per kernel). */
int xv_set_option(xv_handle* h, const char* name, int value);

/* XV_PREC_F16X3 range guard.  Every kernel that converts a value to the fp16 split format records whether it was
 * beyond +-65504 (or NaN).  Returns 1 if that happened in any xv_forward since the last reset (the results of those
 * forwards are not valid: ReLU turns the NaNs that an overflow produces into zeros, so the outputs can look finite),
 * 0 otherwise, or a negative status.  Synchronous device-to-host copy: call it after the results have been fetched. */
int xv_check_overflow(xv_handle* h, int reset);

/* The same guard without a host synchronisation (the driver's software pipeline, egs/voxceleb/v1/nnet/lib/extract.py:63-94
 * batched): copies the two flag words to `host_flags` (2 x int32; pinned host memory makes the copy truly asynchronous)
 * behind everything enqueued on `stream` so far and clears them, in stream order.  Once the stream has reached that
 * point, xv_flags_decode(host_flags) gives 0 = in range, 1 = a value beyond the fp16 range was converted (as above),
 * 2 = an utterance staged since the last clear had every input feature below 2^-8 in magnitude (and not all zero): the
 * low halves of the fp16 split are subnormal there and its outputs lose precision silently (~2^-11 relative on frame-level
 * endpoints) -- rescale the features or use XV_PREC_BF16X3.  The test is per utterance (a batch-wide maximum would let one
 * small utterance among ordinary ones through).
 * Hidden activations have no flag: each layer's split copy is kept at a power-of-two scale derived from the rms of its
 * batch-normalisation gamma / beta (csrc/api_weights.hip, act_exponent), which keeps channels of ordinary magnitude clear of
 * both ends of the fp16 range; per-channel spread inside a 32-channel block is what XV_PREC_F16F6's block scales cannot
 * hold, and xv_finalize demotes such layers (xv_layer_two_unit).  xv_check_overflow returns the same codes. */
int xv_flags_async(xv_handle* h, int32_t* host_flags, void* stream);
int xv_flags_decode(const int32_t* host_flags);

/* endpoints[...] key -> node id (model/trainer.py:380 `endpoints[params.embedding_node]`).
 * Returns the id (>= 0) or XV_ERR_INVALID for a name the graph does not define. */
int xv_node_id(const xv_handle* h, const char* endpoint_name);

/* XV_PREC_F16F6: 1 if the layer that produces `endpoint_name` (any of its stage endpoints, e.g. "tdnn3_conv" / "tdnn3_bn" /
 * "tdnn3_relu"; a ResNet block output names the block's second convolution, "<block>_relu0" its first convolution and
 * "<block>_short" the projection shortcut of an `a` block) runs on the two-unit kernel, 0 if it runs on the
 * three-unit kernels (other precisions, layers the two-unit kernel does not cover, and layers xv_finalize demoted because the
 * magnitudes inside one of their 32-channel blocks -- BN-folded scale / shift of the input channels, |w| of a K group -- are too
 * far apart for the block-scaled fp6 cross terms).  XV_ERR_INVALID for a name that is not a layer endpoint, XV_ERR_STATE before
 * xv_finalize.  Read-only. */
int xv_layer_two_unit(const xv_handle* h, const char* endpoint_name);

/* Number of frames of temporal context the node consumes (tdnn: 14 for everything at or past
 * tdnn3; etdnn: 22 at or past tdnn7); an utterance needs more than this many frames. */
int xv_node_context(const xv_handle* h, int node_id);

/* Batch geometry.  `frame_offsets` (host, B+1 ascending int32, [0] == 0) delimits the B
 * utterances inside the packed feature matrix.  Builds the device-side row maps once, so
 * xv_forward for this geometry is launch-only.  The index arrays are filled by work enqueued
 * on `stream` (no host synchronisation; device buffers are recycled from destroyed plans of the
 * handle, so a stream of ragged batches costs no hipMalloc / hipFree per batch). */
int xv_plan_create(xv_handle* h, const int32_t* frame_offsets, int batch, int node_id, void* stream,
                   xv_plan** out);
int xv_plan_query(const xv_plan* p, xv_plan_info* info);
void xv_plan_destroy(xv_plan* p);

/* sess.run(self.embeddings, {features, is_training: False}) (model/trainer.py:909).
 *   feats_dev : device fp32, packed frames [in_frames, feat_ld]; the first feat_dim columns
 *               are used (trainer.py:906-907 drops extra columns), feat_ld >= feat_dim.
 *   out_dev   : device fp32 [out_rows, out_cols], row-major, out_capacity = element count.
 *   workspace : device scratch >= workspace_bytes, 256-byte aligned.
 *   stream    : hipStream_t (torch.cuda.current_stream().cuda_stream), NULL = default. */
int xv_forward(xv_handle* h, const xv_plan* p, const float* feats_dev, int feat_ld, float* out_dev,
               int64_t out_capacity, void* workspace, int64_t workspace_bytes, void* stream);

/* Per-kernel timing with hipEvents on the launch stream, for bench.py (roofline numbers).
 * Between xv_profile_begin and xv_profile_end every xv_forward on this handle brackets each
 * kernel launch with two events from a pool of `max_events` (no host synchronisation; forwards
 * that no longer fit in the pool run unprofiled).  xv_profile_end synchronises on the recorded
 * events and returns one record per distinct kernel launch shape: mean launch duration over the
 * profiled forwards and the ALGORITHMIC flops / bytes of one launch (2*M*N*K; inputs + outputs +
 * weights once).  Returns the record count (>= 0) or a negative xv_status. */
typedef struct {
  char name[48];
  float ms;          /* mean duration of one launch                                        */
  int32_t launches;  /* launches averaged                                                  */
  int64_t flops;
  int64_t bytes;
} xv_kernel_time;
int xv_profile_begin(xv_handle* h, int max_events);
int xv_profile_end(xv_handle* h, xv_kernel_time* entries, int max_entries, int* n_forwards);

/* ---- feature front-end on the GPU (csrc/frontend.hip): what the reference runs as Kaldi binaries in
 * front of extract.py (egs/voxceleb/v1/nnet/run_extract_embeddings.sh:47),
 *   apply-cmvn-sliding --norm-vars=false --center=true --cmn-window=W  |  select-voiced-frames.
 * feats_dev [in_frames, ld] (first `dim` columns), frame_offsets_dev [B+1] (device), src_rows_dev
 * [out_rows]: input row of every kept frame (ascending inside an utterance; the host derives it from the
 * VAD decisions), scratch_dev: (in_frames + B) * dim doubles.  cmn_window 0 = selection only.  Writes out_dev [out_rows, dim] float32. */
int xv_frontend_cmn_select(int device, const float* feats_dev, int ld, int dim, const int32_t* frame_offsets_dev,
                           int batch, const int32_t* src_rows_dev, int64_t out_rows, int cmn_window, int center,
                           int min_window, double* scratch_dev, float* out_dev, void* stream);

/* ---- MFCC features and energy VAD on the GPU (csrc/mfcc.hip): the first step of the reference recipe
 * (egs/voxceleb/v1/run.sh:57-65), steps/make_mfcc.sh and sid/compute_vad_decision.sh.  The algorithm is Kaldi's as published
 * and is written out in the header of csrc/mfcc.hip; **parity unpinned**.  Field names and defaults are the options of Kaldi's
 * compute-mfcc-feats; a field set to a value this library cannot honour is refused by xv_mfcc_create with a message
 * (xv_last_error(NULL)): dither != 0 (Kaldi's default 1.0 is random noise; here features are deterministic), htk_compat,
 * round_to_power_of_two = 0, a padded frame length other than 256 or 512 samples, num_mel_bins > 64, frame shift > frame length. */
enum { XV_WINDOW_POVEY = 0, XV_WINDOW_HAMMING = 1, XV_WINDOW_HANNING = 2, XV_WINDOW_RECTANGULAR = 3 };
typedef struct {
  int32_t struct_size;             /* sizeof(xv_mfcc_opts)                         */
  float sample_frequency;          /* --sample-frequency          16000            */
  float frame_length_ms;           /* --frame-length              25               */
  float frame_shift_ms;            /* --frame-shift               10               */
  float preemphasis_coefficient;   /* --preemphasis-coefficient   0.97             */
  int32_t remove_dc_offset;        /* --remove-dc-offset          1                */
  int32_t window_type;             /* --window-type               XV_WINDOW_POVEY  */
  int32_t round_to_power_of_two;   /* --round-to-power-of-two     1                */
  int32_t snip_edges;              /* --snip-edges                1                */
  float dither;                    /* --dither                    0 (Kaldi: 1.0)   */
  int32_t num_mel_bins;            /* --num-mel-bins              23               */
  float low_freq;                  /* --low-freq                  20               */
  float high_freq;                 /* --high-freq                 0 (<= 0: Nyquist + value) */
  int32_t num_ceps;                /* --num-ceps                  13               */
  float cepstral_lifter;           /* --cepstral-lifter           22               */
  int32_t use_energy;              /* --use-energy                1                */
  float energy_floor;              /* --energy-floor              0                */
  int32_t raw_energy;              /* --raw-energy                1                */
  int32_t htk_compat;              /* --htk-compat                0 (1 is refused) */
} xv_mfcc_opts;
typedef struct xv_mfcc xv_mfcc;
/* xv_mfcc_create / xv_mfcc_destroy: the tables of one option set (window, FFT twiddles, mel bank, DCT x lifter; built in double,
 *   rounded once to fp32) on `device`.  Option checks come before the first HIP call.
 * xv_mfcc_num_frames: frames compute-mfcc-feats yields for an utterance of num_samples samples (< 0: XV_ERR_INVALID).
 * xv_mfcc_compute = `compute-mfcc-feats`: wave_dev holds the int16 samples of `batch` utterances back to back, utterance b at
 *   [sample_offsets_dev[b], sample_offsets_dev[b + 1]); frame_offsets_dev [batch + 1] are the prefix sums of xv_mfcc_num_frames.
 *   Writes the num_ceps features of frame t of utterance b to feats_dev[(frame_offsets[b] + t) * ld .. ], ld >= num_ceps; other
 *   columns are left alone.  fp32, no atomics: repeated runs are bit-identical.
 * xv_vad_energy = `compute-vad-decision`: column 0 of feats_dev is the log energy; writes one float (0 or 1) per frame to
 *   vad_dev[frame_offsets[b] + t].  The mean is accumulated in double in a fixed order. */
int xv_mfcc_create(const xv_mfcc_opts* opts, int device, xv_mfcc** out);
void xv_mfcc_destroy(xv_mfcc* m);
int64_t xv_mfcc_num_frames(const xv_mfcc* m, int64_t num_samples);
int xv_mfcc_compute(xv_mfcc* m, const int16_t* wave_dev, const int64_t* sample_offsets_dev, const int32_t* frame_offsets_dev,
                    int batch, float* feats_dev, int64_t ld, void* stream);
int xv_vad_energy(int device, const float* feats_dev, int64_t ld, const int32_t* frame_offsets_dev, int batch, float threshold,
                  float mean_scale, int context, float proportion, float* vad_dev, void* stream);

/* ---- Fbank features on the GPU (csrc/mfcc.hip): steps/make_fbank.sh --fbank-config conf/fbank.conf of the ResNet recipe
 * (egs/voxceleb/v3/run.sh:54), Kaldi's compute-fbank-feats as published; written out in the header of csrc/mfcc.hip next to the
 * MFCC, **parity unpinned**.  The frame fields mean what they mean in xv_mfcc_opts and the same values are refused, with the
 * same messages. */
typedef struct {
  int32_t struct_size;             /* sizeof(xv_fbank_opts)                        */
  float sample_frequency;          /* --sample-frequency          16000            */
  float frame_length_ms;           /* --frame-length              25               */
  float frame_shift_ms;            /* --frame-shift               10               */
  float preemphasis_coefficient;   /* --preemphasis-coefficient   0.97             */
  int32_t remove_dc_offset;        /* --remove-dc-offset          1                */
  int32_t window_type;             /* --window-type               XV_WINDOW_POVEY  */
  int32_t round_to_power_of_two;   /* --round-to-power-of-two     1                */
  int32_t snip_edges;              /* --snip-edges                1                */
  float dither;                    /* --dither                    0 (Kaldi: 1.0)   */
  int32_t num_mel_bins;            /* --num-mel-bins              23 (3..64)       */
  float low_freq;                  /* --low-freq                  20               */
  float high_freq;                 /* --high-freq                 0 (<= 0: Nyquist + value) */
  int32_t use_energy;              /* --use-energy                0                */
  float energy_floor;              /* --energy-floor              0                */
  int32_t raw_energy;              /* --raw-energy                1                */
  int32_t htk_compat;              /* --htk-compat                0 (1 is refused) */
  int32_t use_log_fbank;           /* --use-log-fbank             1                */
  int32_t use_power;               /* --use-power                 1                */
} xv_fbank_opts;
typedef struct xv_fbank xv_fbank;
/* xv_fbank_create / xv_fbank_destroy: the tables of one option set on `device`.  Option checks come before the first HIP call.
 * xv_fbank_num_frames: as xv_mfcc_num_frames.  xv_fbank_num_feats: num_mel_bins + use_energy.
 * xv_fbank_compute = `compute-fbank-feats`: operands as for xv_mfcc_compute.  Writes the num_feats features of frame t of
 *   utterance b to feats_dev[(frame_offsets[b] + t) * ld .. ], ld >= num_feats (column 0 is the log energy with use_energy);
 *   other columns are left alone.  log_energy_dev may be NULL; otherwise log_energy_dev[frame_offsets[b] + t] receives the
 *   frame's log energy under raw_energy and energy_floor, whatever use_energy says: the bits xv_mfcc_compute puts in
 *   coefficient 0 with use_energy and the same frame, raw_energy and energy_floor fields, so xv_vad_energy (ld = 1) decides on
 *   it as it does on an MFCC file.  fp32, no atomics: repeated runs are bit-identical. */
int xv_fbank_create(const xv_fbank_opts* opts, int device, xv_fbank** out);
void xv_fbank_destroy(xv_fbank* m);
int64_t xv_fbank_num_frames(const xv_fbank* m, int64_t num_samples);
int xv_fbank_num_feats(const xv_fbank* m);
int xv_fbank_compute(xv_fbank* m, const int16_t* wave_dev, const int64_t* sample_offsets_dev, const int32_t* frame_offsets_dev,
                     int batch, float* feats_dev, int64_t ld, float* log_energy_dev, void* stream);

/* ---- post-step on the GPU (csrc/post.hip): what the reference runs as Kaldi binaries behind extract.py
 * (egs/voxceleb/v1/nnet/run_extract_embeddings.sh:80-103).
 * xv_length_normalize = `ivector-normalize-length [--scaleup=false]` (:86,88,101): out[r] = x[r] / ratio,
 *   ratio = ||x[r]||_2 (scaleup 0) or ||x[r]||_2 / sqrt(dim) (scaleup 1); a zero vector is copied unchanged.
 * xv_speaker_mean = `ivector-mean ark:spk2utt` (:87,92): speaker s owns utt_index[spk_offsets[s] .. spk_offsets[s+1])
 *   (row numbers of x, spk2utt order, utterances without a vector already removed by the host); out[s] = their
 *   float32 sum in that order times float(1 / count); a speaker without utterances gets zeros (the host drops it).
 * x_dev [rows, ldx], out_dev [rows | num_speakers, ldo] device float32; in-place (out_dev == x_dev) is allowed for
 * xv_length_normalize. */
int xv_length_normalize(int device, const float* x_dev, int64_t ldx, int64_t rows, int dim, int scaleup, float* out_dev,
                        int64_t ldo, void* stream);
int xv_speaker_mean(int device, const float* x_dev, int64_t ldx, int dim, const int32_t* spk_offsets_dev,
                    const int32_t* utt_index_dev, int64_t num_speakers, float* out_dev, int64_t ldo, void* stream);

/* ---- cosine scoring on the GPU (csrc/score.hip): the back-end the reference runs as Kaldi binaries and as a numpy
 * double loop.  All arithmetic is fp32 with exact products; a score of two prepared (unit) rows of length d is within
 * (d + 8) * 2^-24 of the exact value.  Rows are device float32; every argument check comes before the first HIP call.
 * xv_score_prepare = `ivector-subtract-global-mean` | `transform-vec` | `ivector-normalize-length`
 *   (egs/voxceleb/v1/run.sh:404-407) and the normalisation of misc/utils.py:317, each step optional and in this order:
 *   y = x - mean (mean_dev [d_in] or NULL); y = T y (transform_dev [d_out, t_cols] or NULL; t_cols == d_in, or d_in + 1 with
 *   the last column an offset, i.e. the input extended by a constant 1); y / sqrt(sum y^2 + eps) when `normalize`
 *   (eps 0: Kaldi, a zero row stays zero; eps 1e-12: misc/utils.py).  Without a transform d_out == d_in and out_dev may be
 *   x_dev; with one, d_in <= 2048 (XV_ERR_UNSUPPORTED beyond) and out_dev is a different buffer.
 * xv_score_matrix = the score matrix of misc/utils.py:318 (`np.dot(embeddings, np.transpose(embeddings))`), for two sets:
 *   out[i, j] = a[i] . b[j], a [n, d], b [m, d], out [n, ldo].
 * xv_score_pairs = `ivector-compute-dot-products` (egs/voxceleb/v1/run.sh:362-365,408): out[k] = a[ia[k]] . b[ib[k]].
 *   The caller checks 0 <= ia[k] < n, 0 <= ib[k] < m on the host (tf_kaldi_speaker_amd.scoring raises XV_ERR_INVALID); an
 *   index that slips through is never followed: its score is NaN.  Repeats are bit-identical.
 * xv_score_histogram = the double loop of misc/utils.py:320-327 without the matrix: every score is counted in
 *   hist_same[bin] (labels_a[i] == labels_b[j]) or hist_diff[bin], bin = clamp(floor((s + 1) * nbins / 2), 0, nbins - 1),
 *   nbins a power of two in 256..65536.  `self` (a == b, same labels): only the pairs i < j.  The histograms [nbins] are
 *   uint64 and are ADDED to (the caller zeroes them); the counts are exact and independent of the order of execution.
 * 1 <= d <= 2048 in the last three, anything else is XV_ERR_UNSUPPORTED. */
int xv_score_prepare(int device, const float* x_dev, int64_t ldx, int64_t n, int d_in, const float* mean_dev,
                     const float* transform_dev, int64_t ldt, int d_out, int t_cols, int normalize, float eps, float* out_dev,
                     int64_t ldo, void* stream);
int xv_score_matrix(int device, const float* a_dev, int64_t lda, int64_t n, const float* b_dev, int64_t ldb, int64_t m, int d,
                    float* out_dev, int64_t ldo, void* stream);
int xv_score_pairs(int device, const float* a_dev, int64_t lda, int64_t n, const float* b_dev, int64_t ldb, int64_t m, int d,
                   const int32_t* ia_dev, const int32_t* ib_dev, int64_t npairs, float* out_dev, void* stream);
int xv_score_histogram(int device, const float* a_dev, int64_t lda, int64_t n, const int32_t* labels_a_dev, const float* b_dev,
                       int64_t ldb, int64_t m, const int32_t* labels_b_dev, int d, int self, int nbins, uint64_t* hist_same_dev,
                       uint64_t* hist_diff_dev, void* stream);

/* ---- PLDA scoring on the GPU (csrc/score.hip): scoring with a trained Kaldi `Plda` (mean, transform, psi), the last line of
 * every recipe of the reference (`ivector-plda-scoring`, egs/voxceleb/v1/run.sh:410-426, egs/sre/v1/run.sh:415-491).  Kaldi is
 * absent from the reference tree: these restate plda.cc as published (**parity unpinned**).  Training is the next block (csrc/backend.hip).
 * With c = n psi / (n psi + 1) and v = 1 + psi / (n psi + 1) the log likelihood ratio of plda.cc is
 *   s(i, j) = sum_d A_id t_jd + sum_d W_id t_jd^2 + rho_i,  A = e c / v,  W = (1 / (1 + psi) - 1 / v) / 2,
 *   rho = sum_d [log(1 + psi) - log v] / 2 - sum_d e^2 c^2 / v / 2
 * (tf_kaldi_speaker_amd.plda builds the per-n tables in float64).  All products are exact fp32 with fp32 accumulation, as in the
 * cosine entry points; rho / tau are accumulated in double and rounded once.
 * xv_plda_prepare = `Plda::TransformIvector` (plda.cc) of n rows, and the packed operands of the scoring calls:
 *   u = T [x; 1] (transform_dev [d, d_in + 1], the last column holding -transform * mean; NULL: x is u already, d_in == d);
 *   y = u sqrt(d / sum_d u_d^2 inv_d) (norm 1: --normalize-length=true), u sqrt(d) / ||u|| (norm 2:
 *   --simple-length-normalization=true) or u (norm 0); a zero row stays zero.  tables_dev [num_tables, 4, d] doubles holds per
 *   distinct n the vectors inv, p, q, w and logdet_dev [num_tables] (or NULL: 0) a constant; table_index_dev [n] picks the
 *   table of a row (NULL: table 0).  Outputs, each optional: rows_dev [n, ldr] = y; packed_dev [n, ldp] = y p in columns
 *   0..d-1 and, with pack_second, w (side 0, enrolment) or y^2 (side 1, test) in columns d..2d-1; bias_dev [n] =
 *   logdet + sum_d q_d y_d^2.  rows_dev == x_dev is allowed without a transform.
 * xv_plda_matrix = `Plda::LogLikelihoodRatio` over two sets: out[i, j] = a[i] . b[j] + rho[i] + tau[j], a [n, k], b [m, k] packed
 *   rows (k = d, or 2 d for an enrolment set of mixed n), tau_dev NULL = 0.
 * xv_plda_pairs = `ivector-plda-scoring` over a trial list: out[t] = a[ia[t]] . b[ib[t]] + rho[ia[t]] + tau[ib[t]]; indices as in
 *   xv_score_pairs (checked by the caller, never followed out of range: NaN); repeats are bit-identical.
 * xv_plda_histogram = xv_score_histogram over the PLDA scores of a x b and a caller-given range:
 *   bin = clamp(floor((s - lo) * nbins / (hi - lo)), 0, nbins - 1), so the end bins also hold what falls outside [lo, hi).
 * 1 <= k <= 2048 in the last three, 1 <= d, d_in <= 2048 in the first; anything else is XV_ERR_UNSUPPORTED. */
int xv_plda_prepare(int device, const float* x_dev, int64_t ldx, int64_t n, int d_in, const float* transform_dev, int64_t ldt,
                    int d, int norm, int side, int pack_second, const double* tables_dev, const double* logdet_dev,
                    int num_tables, const int32_t* table_index_dev, float* rows_dev, int64_t ldr, float* packed_dev, int64_t ldp,
                    float* bias_dev, void* stream);
int xv_plda_matrix(int device, const float* a_dev, int64_t lda, int64_t n, const float* rho_dev, const float* b_dev, int64_t ldb,
                   int64_t m, const float* tau_dev, int k, float* out_dev, int64_t ldo, void* stream);
int xv_plda_pairs(int device, const float* a_dev, int64_t lda, int64_t n, const float* rho_dev, const float* b_dev, int64_t ldb,
                  int64_t m, const float* tau_dev, int k, const int32_t* ia_dev, const int32_t* ib_dev, int64_t npairs,
                  float* out_dev, void* stream);
int xv_plda_histogram(int device, const float* a_dev, int64_t lda, int64_t n, const float* rho_dev, const int32_t* labels_a_dev,
                      const float* b_dev, int64_t ldb, int64_t m, const float* tau_dev, const int32_t* labels_b_dev, int k, double lo,
                      double hi, int nbins, uint64_t* hist_same_dev, uint64_t* hist_diff_dev, void* stream);

/* ---- score normalisation on the GPU (csrc/score.hip): Z/T/S-norm with adaptive top-K cohorts.  The reference has no such step
 * (egs/sre/v1/run.sh:13, "In the future, we will add score-normalization"), so this is **parity unpinned**; the oracle is
 * tests/helpers/ref_snorm.py.  Definitions:
 *   e is an enrolment row and t is a test row.  The cohort has rows c_1..c_m.
 *   score() is either the cosine of prepared rows or the PLDA log likelihood ratio.
 *   S_e = { score(e, c_j) }: for PLDA the cohort stands on the *test* side.
 *   S_t = { score(c_j, t) }: for PLDA the cohort stands on the *enrolment* side, num_utts 1.
 *   top_K(S) is the K largest values of S, with multiplicity.  Ties at the boundary are harmless, because equal values
 *   contribute equally.  mu(S) is the mean of top_K(S).  sigma(S) is the population standard deviation (divide by K, numpy's
 *   default), computed centred on mu.
 *   top_k = 0 means K = all eligible columns: plain Z-norm / T-norm.  Otherwise K_eff = min(top_k, eligible).  This is adaptive
 *   S-norm in its "AS-norm1" form: each side picks its own top-K cohort.
 *   z: (s - mu(S_e)) / sigma(S_e).  t: (s - mu(S_t)) / sigma(S_t).  s: (z + t) / 2.
 *   Optional exclusion labels: a column whose label equals the row's label is not eligible.  Use this when the cohort is drawn
 *   from the set being scored, or holds the same speaker.
 *   If K_eff = 0, mean and std are NaN.  If K_eff = 1, or all selected values are equal, std is exactly 0.  This is why the
 *   variance is taken centred (two-pass), not as E[s^2] - E[s]^2.
 *   AS-norm2 (cohort chosen by the other side of the trial) is out of scope and is not offered.
 * xv_cohort_stats = per row i of a [n, k]: mean_dev[i] = mu, std_dev[i] = sigma and count_dev[i] = K_eff (count_dev may be NULL) of
 *   the scores a[i] . b[j] + row_bias[i] + col_bias[j] against the m rows of b [m, k] (either bias NULL: 0).  One entry point
 *   serves cosine (no biases) and PLDA (the operands of xv_plda_matrix); the form is symmetric in its two sides, so the statistics
 *   per test row over cohort enrolments are the same call with the operands swapped.  Every score is produced by the tile kernel
 *   of xv_score_matrix / xv_plda_matrix and is bit-identical to what those calls write for the same operand order (the biases
 *   are added as (a . b + row_bias) + col_bias).  Selection is an exact radix select per row (no sampling); mean and centred sum
 *   of squares are accumulated in double in a fixed order without floating-point atomics and rounded once: repeats are
 *   bit-identical.  labels_a_dev [n] / labels_b_dev [m] are both NULL (no exclusion) or both given.
 *   The scores pass through ws_dev in panels of whole 128-row tile rows; xv_cohort_stats_workspace(n, m, top_k) is the least
 *   ws_bytes (one 128-row panel of m scores, rows padded to 4 floats) and XV_ERR_WORKSPACE is returned below it.  The result is
 *   bit-identical for every legal ws_bytes: more workspace only means more rows per launch.
 *   1 <= k <= 2048 (XV_ERR_UNSUPPORTED otherwise), 0 <= top_k <= m, m < 2^31, n < 2^31 (XV_ERR_INVALID otherwise); all argument
 *   checks come before the first HIP call.  n = 0 returns XV_OK and touches nothing. */
int64_t xv_cohort_stats_workspace(int64_t n, int64_t m, int top_k);
int xv_cohort_stats(int device, const float* a_dev, int64_t lda, int64_t n, const float* row_bias_dev /* NULL: 0 */,
                    const int32_t* labels_a_dev /* NULL: no exclusion */, const float* b_dev, int64_t ldb, int64_t m,
                    const float* col_bias_dev /* NULL: 0 */, const int32_t* labels_b_dev, int k, int top_k,
                    float* mean_dev, float* std_dev, int32_t* count_dev /* K_eff per row; may be NULL */,
                    void* ws_dev, int64_t ws_bytes, void* stream);

/* ---- identification on the GPU (csrc/score.hip): top-K search of a gallery, cosine and PLDA.  The reference has no
 * identification step, so this is **parity unpinned**; the rule below is the specification and tests/helpers/ref_topk.py states it
 * in numpy.  Definitions:
 *   The score of (i, j) is (a[i] . b[j] + row_bias[i]) + col_bias[j] over a [n, k] and b [m, k] (either bias NULL: 0).  It is
 *   produced by the tile kernel of xv_score_matrix / xv_plda_matrix and is bit-identical to what those calls write for the same
 *   operand order.  One entry point serves cosine (no biases) and PLDA (the packed operands, rho and tau of xv_plda_matrix).
 *   Column j is eligible for row i unless both label arrays are given and labels_a[i] == labels_b[j].  labels_a_dev [n] /
 *   labels_b_dev [m] are both NULL (no exclusion) or both given.  This is how a set is searched against itself without each
 *   row finding itself.
 *   K_eff = min(top_k, eligible columns).  Row i of scores_dev / index_dev [n, ldo] holds the K_eff eligible columns with the
 *   largest scores, by score descending and, among equal scores, by column ascending; ties at the selection boundary go to the
 *   lowest columns too.  -0.0 and +0.0 are equal scores.  Positions K_eff .. top_k - 1 hold -inf and -1; nothing is written
 *   past column top_k - 1 of a row.  count_dev[i] = K_eff (count_dev may be NULL).
 *   Order is that of the integer image the select uses (sign-flipped bits of the float): a NaN with the sign bit clear sorts
 *   above +inf and one with the sign bit set below -inf, by payload; NaN scores of equal bits tie like any other.
 *   The result is a pure function of the inputs: an exact radix select per row, a compaction whose slots come from a prefix
 *   scan in column order (no atomic counter) and a sort of distinct (score, column) keys.  Repeats are bit-identical.
 *   The scores pass through ws_dev in panels of whole 128-row tile rows, as in xv_cohort_stats;
 *   xv_score_topk_workspace(n, m, top_k) is the least ws_bytes (one 128-row panel of m scores, rows padded to 4 floats; it
 *   depends on m alone) or XV_ERR_INVALID for arguments xv_score_topk refuses.  The result is the same bits for every legal
 *   ws_bytes: more workspace only means more rows per launch.  One workgroup selects one row, so for a gallery of many
 *   thousands of rows several panels (512 rows per launch or more) are considerably faster than the least (profiles/scoring.md).
 *   1 <= k <= 2048 and 1 <= top_k <= 1024 (XV_ERR_UNSUPPORTED otherwise; top_k > m is legal, the row is padded); m < 2^31,
 *   n < 2^31, lda, ldb >= k, ldo >= top_k, the label arrays as above (XV_ERR_INVALID otherwise); ws_bytes below the least is
 *   XV_ERR_WORKSPACE.  Every argument check comes before the first HIP call.  n = 0 returns XV_OK and touches nothing; m = 0
 *   writes the padding. */
int64_t xv_score_topk_workspace(int64_t n, int64_t m, int top_k);
int xv_score_topk(int device, const float* a_dev, int64_t lda, int64_t n, const float* row_bias_dev /* NULL: 0 */,
                  const int32_t* labels_a_dev /* NULL: no exclusion */, const float* b_dev, int64_t ldb, int64_t m,
                  const float* col_bias_dev /* NULL: 0 */, const int32_t* labels_b_dev, int k, int top_k,
                  float* scores_dev /* [n, ldo] */, int32_t* index_dev /* [n, ldo] */, int64_t ldo,
                  int32_t* count_dev /* K_eff per row; may be NULL */, void* ws_dev, int64_t ws_bytes, void* stream);

/* ---- speaker clustering on the GPU (csrc/cluster.hip): average-linkage agglomerative clustering per recording, the step of
 * Kaldi's diarization/cluster.sh (agglomerative-cluster over a dense cosine or PLDA score matrix).  The reference has no
 * clustering step, so this is **parity unpinned**; the rule below is the specification and tests/helpers/ref_cluster.py states
 * it in numpy.  One group is one recording with n rows:
 *   Input: a score matrix s [n, ld] float32, larger = more similar, ld = max(4, n rounded up to 4).  Only entries with column >
 *   row are ever read: s(i, j), i < j, is the similarity of rows i and j.  The diagonal, the lower triangle and the padding
 *   columns may hold anything, NaN included, and are never written.
 *   State: every row starts as a cluster of size 1; a cluster is named by its lowest member row.  S(A, B) is a float32 sum that
 *   starts as s(a, b).  When clusters a < b merge, the merged cluster keeps the name a and for every other live cluster k
 *   S(a, k) <- S(a, k) + S(b, k), one float32 addition: every sum is a fixed chain of float32 additions given by the merge order.
 *   Linkage: L(A, B) = double(S(A, B)) / double(|A| * |B|), the size product formed in int64, one correctly rounded division.
 *   |L - exact mean of the original scores| <= (n - 2) 2^-24 (1 + small) max|s| (derived in the header of csrc/cluster.hip).
 *   Step: among all live pairs a < b whose L is not NaN take the largest L; among equal L (-0.0 equals +0.0) the lowest a, then
 *   the lowest b.  Stop without merging if there is no such pair, or clusters <= target, or not (L >= threshold).  Otherwise
 *   merge and record (a, b, L).  The loop is a for over at most n - 1 steps.
 *   Output: labels[i] = the cluster of row i, clusters numbered 0, 1, ... in the order of their lowest rows; num_clusters; the
 *   merge log merge_a, merge_b (int32) and merge_height (double, the L of the step), whose positions past the merges performed
 *   hold -1 / -1 / NaN.  Average linkage has no inversions beyond rounding, so stopping at a threshold equals cutting the
 *   finished dendrogram, and the log lets a caller re-cut on the host.
 *   threshold is in score terms (Kaldi's --threshold negated when the scores are negated costs); -inf means none.  target_host[g]
 *   >= 1 is the number of clusters to stop at (reco2num_spk); NULL means 1 everywhere; a target of n or more merges nothing.
 *   The result is a pure function of the group's own matrix, threshold and target: the same bits on every repeat, alone or
 *   inside any batch, for every legal ws_bytes.
 * Layout: the group matrices lie back to back in s_dev, group g at the float offset sum_{h<g} xv_ahc_matrix_floats(rows[h])
 *   (xv_ahc_matrix_floats(n) = n * ld(n); 0 for n <= 0).  s_dev is the working matrix: the upper triangles are unspecified on
 *   return.  labels_dev, merge_a_dev, merge_b_dev and merge_height_dev are packed by the prefix sum of rows: a group has n slots
 *   in each (n - 1 possible merges plus one slot that is always -1 / -1 / NaN).  num_clusters_dev [num_groups].  rows_host and
 *   target_host are host arrays and are consumed before the call returns; the library copies the group table into ws_dev,
 *   stream-ordered.  xv_ahc_workspace(num_groups, rows_host) is the least ws_bytes (32 bytes per group rounded up to 256), or
 *   the code xv_ahc returns for the same rows (XV_ERR_INVALID, XV_ERR_UNSUPPORTED).  ws_dev must be 8-byte aligned
 *   (XV_ERR_INVALID otherwise): it holds 64-bit offsets.
 * One 256-thread workgroup clusters one group, the large groups first; no workgroup waits for another and there is no atomic.
 *   A row-best cache (per live row the best partner to its right) lives in LDS, 16 bytes per row, which bounds n:
 *   0 <= rows[g] <= 8192, above that XV_ERR_UNSUPPORTED.  A negative row count, target < 1 or a NaN threshold is
 *   XV_ERR_INVALID; too little workspace XV_ERR_WORKSPACE.  Every argument check comes before the first HIP call and the outputs
 *   are untouched on any error.  num_groups = 0 returns XV_OK and touches nothing; a group of 0 rows writes only
 *   num_clusters = 0; a group of 1 row gets label 0, count 1 and an empty log. */
int64_t xv_ahc_matrix_floats(int64_t n);
int64_t xv_ahc_workspace(int64_t num_groups, const int32_t* rows_host);
int xv_ahc(int device, float* s_dev, const int32_t* rows_host, const int32_t* target_host /* NULL: 1 */, int64_t num_groups,
           double threshold, int32_t* labels_dev, int32_t* num_clusters_dev, int32_t* merge_a_dev, int32_t* merge_b_dev,
           double* merge_height_dev, void* ws_dev, int64_t ws_bytes, void* stream);

/* ---- per-recording PCA adaptation of a PLDA model on the GPU (csrc/plda_adapt.hip): what Kaldi's diarization recipe does in
 * front of every recording's score matrix (`ivector-plda-scoring-dense --target-energy`: EstPca, ApplyPca,
 * Plda::ApplyTransform).  Kaldi is absent from the reference tree, so this is **parity unpinned**; the rule below is the
 * specification and tests/helpers/ref_plda_adapt.py states it in numpy.  All arithmetic is double (Kaldi's PCA is float).
 * The global model is (m, A, psi) with A = Plda.transform: within-class covariance A^-1 A^-T, between-class A^-1 diag(psi) A^-T.
 * One group is one recording with n float32 rows x_1 .. x_n of length d:
 *   1. mu = (the sum of the rows in double, in row order) / n;  C = (1 / n) sum (x - mu)(x - mu)^T in double, every entry one
 *      chain of fused multiply-adds in row order and one division: the bound of xv_gram_f64 with c = mu, plus the division.
 *   2. C = V diag(lambda) V^T, lambda_0 >= lambda_1 >= ... >= lambda_{d-1}.
 *   3. k = the least k >= 1 with lambda_0 + .. + lambda_{k-1} > target_energy * trace, trace = the sum of all lambda in
 *      descending order; r = min(k + 1, d) (the published loop keeps one direction more than it needs); no such k: r = d.
 *   4. P = the first r eigenvectors as rows [r, d].
 *   5. M = P A^-1, W' = M M^T, B' = M diag(psi) M^T.
 *   6. W' = L L^T (Cholesky), K = L^-1 B' L^-T = U diag(psi') U^T, psi' descending (and clamped at 0 from below).
 *   7. A' = U^T L^-1; the adapted affine is T = [A' P | -A' P m], [r, d + 1]: u = T [x; 1] has within-class covariance I and
 *      between-class covariance diag(psi'), and scoring goes on as with any Plda of dimension r.
 *   8. Every row of P (before step 5) and every row of T is scaled by +-1 so that its entry of largest magnitude, the lowest
 *      column among equals, is positive.  Scores do not depend on these signs nor on the basis inside an eigenspace.
 *   9. Fallback: dim = 0 (the caller scores the group with the global model) when n < 2, when trace is not > 0, when the
 *      Cholesky meets a pivot that is not > 0, or when an eigen-iteration has not converged after 30 sweeps.
 *   The outputs of a group are a pure function of its own rows, the model and target_energy: the same bits on every repeat,
 *   alone or in any batch, in any group order, for every legal ws_bytes.  No floating-point atomics.
 * Eigen-iteration: two-sided cyclic Jacobi, round-robin pairs, Rutishauser's rotation; a pair is rotated while |a_pq| >
 *   2^-53 ||A||_F / m (m = the dimension rounded up to even) and the iteration ends with the first sweep that rotates nothing.
 * Layout: group g owns the rows offsets[g] .. offsets[g + 1]) of x_dev [*, ldx] (the caller sorts the rows by group);
 *   offsets_host is a host array, consumed before the call returns.  within_factor_dev = A^-1 [d, d], inverted by the caller
 *   in float64.  dim_dev [G] = r or 0; eigval_dev [G, d] = all of lambda, descending, written whenever n >= 2; pca_dev
 *   [G, d, d], rows 0..r-1 = P; affine_dev [G, d, d + 1], rows 0..r-1 = T; psi_out_dev [G, d], entries 0..r-1 = psi'.  What lies
 *   past r, and everything but dim (and eigval) of a fallback group, is unspecified.
 * Workspace: xv_plda_adapt_workspace(G, d) = 256 ceil((16 G + 8) / 256) + 32 m^2 bytes is the least ws_bytes: the group table
 *   and one slot.  One workgroup works in one slot; every further xv_plda_adapt_slot_bytes(d) = 32 m^2 bytes lets one more
 *   group run at a time (up to min(G, 1024); what lies beyond is not used).  On return the int32 pairs at ws_dev + 8 (G + 1) hold, per group, the sweeps the two iterations needed
 *   (-1: cap met; 0: not run or nothing to rotate).  ws_dev must be 8-byte aligned (XV_ERR_INVALID otherwise).
 * 1 <= d <= 256, anything else is XV_ERR_UNSUPPORTED (so does xv_plda_adapt_workspace return).  Offsets that decrease or start
 *   below 0, ldx < d, a target_energy outside (0, 1] or NaN: XV_ERR_INVALID; too little workspace: XV_ERR_WORKSPACE.  Every
 *   argument check comes before the first HIP call and the outputs are untouched on any error.  num_groups = 0 returns XV_OK
 *   and touches nothing. */
int64_t xv_plda_adapt_workspace(int64_t num_groups, int d);
int64_t xv_plda_adapt_slot_bytes(int d);
int xv_plda_adapt(int device, const float* x_dev, int64_t ldx, const int64_t* offsets_host /* [num_groups + 1] */,
                  int64_t num_groups, int d, const double* mean_dev /* [d] */, const double* within_factor_dev /* A^-1 [d, d] */,
                  const double* psi_dev /* [d] */, double target_energy,
                  int32_t* dim_dev /* [G]: r, or 0 = fall back */, double* eigval_dev /* [G, d], all of lambda, descending */,
                  double* pca_dev /* [G, d, d], rows 0..r-1 = P */, double* affine_dev /* [G, d, d + 1], rows 0..r-1 = T */,
                  double* psi_out_dev /* [G, d], entries 0..r-1 = psi' */, void* ws_dev, int64_t ws_bytes, void* stream);

/* ---- VB-HMM resegmentation of clustered x-vectors on the GPU (csrc/vbx.hip): the Bayesian HMM over the x-vector sequence of
 * a recording that diarization recipes run after the first clustering ("VBx": Landini et al., "Bayesian HMM clustering of
 * x-vector sequences", 2022; the function VBx of the published VB_diarization.py).  Neither the reference tree nor Kaldi's
 * x-vector recipe has the step, so this is **parity unpinned**; the rule below is the specification and
 * tests/helpers/ref_vbx.py states it in numpy.  All arithmetic is double.
 * One group is one recording with T >= 1 float32 rows x_0 .. x_{T-1} of length d, in time order, S initial speakers, the affine
 * A [r, d + 1] and psi [r] of the model (for a Plda [transform | -transform mean] and psi; for an adapted model its affine and
 * psi; the first k rows / entries keep k dimensions).  No length normalisation happens inside.
 *   1. u_t = A [x_t; 1];  rho_t = u_t * sqrt(psi);  G_t = -1/2 (sum_k u_tk^2 + r log(2 pi)).
 *   2. Start values: gamma [T, S] with rows >= 0 and pi [S] >= 0 with a positive sum (the caller's duty; not checked).
 *   3. Iteration i = 0, 1, ..:
 *        N_s = sum_t gamma_ts;  invL_sk = 1 / (1 + Fa/Fb N_s psi_k);  alpha_sk = Fa/Fb invL_sk sum_t gamma_ts rho_tk;
 *        logp_ts = Fa (rho_t . alpha_s - 1/2 sum_k (invL_sk + alpha_sk^2) psi_k + G_t);
 *        tr_ij = loop_prob [i = j] + (1 - loop_prob) pi_j;
 *        forward:  lfw_0 = logp_0 + log pi,  lfw_t,j = logp_tj + log sum_i exp(lfw_{t-1},i) tr_ij;
 *        backward: lbw_{T-1} = 0,  lbw_t,i = log sum_j tr_ij exp(logp_{t+1},j + lbw_{t+1},j);
 *        tll = logsumexp_j lfw_{T-1},j;  gamma = exp(lfw + lbw - tll);
 *        ELBO_i = tll + Fb/2 sum_sk (log invL_sk - invL_sk - alpha_sk^2 + 1);
 *        pi_j <- gamma_0j + (1 - loop_prob) pi_j sum_{t>=1} exp(logsumexp_i lfw_{t-1},i + logp_tj + lbw_tj - tll), then
 *        pi <- pi / sum pi (T = 1: the sum over t is empty);
 *        stop after this iteration if i > 0 and ELBO_i - ELBO_{i-1} < epsilon, or if i = max_iters - 1.
 *      epsilon = -inf means "run all max_iters".
 *   4. Outputs: the last gamma and the updated pi; ELBO_0 .. ELBO_{n-1} and n, the rest of the ELBO row NaN; label_t = the
 *      lowest s with the largest gamma_ts.
 *   5. Log-domain sums take their maximum out first (0 when every term is -inf, so that no NaN comes out of finite input);
 *      a speaker with pi_j = 0 has gamma_.j = 0 exactly and stays dead; -inf is a legal log value.
 *   6. tr is a diagonal plus a rank-one matrix and the kernel uses that: with m = max_i lfw_{t-1},i, e_i = exp(lfw_{t-1},i - m)
 *      and E = sum_i e_i the forward step is lfw_t,j = logp_tj + m + log(loop_prob e_j + (1 - loop_prob) pi_j E), the backward
 *      step alike: O(S) per frame, the same sum in another order.
 *   7. The outputs of a group are a pure function of its own rows, start values, model and options: the same bits on every
 *      repeat, alone or in any batch, in any group order, for every legal ws_bytes and whatever the workspace held before.  No
 *      floating-point atomics.
 * Layout: group g owns the rows offsets[g] .. offsets[g + 1]) of x_dev [*, ldx] and the same entries of labels_dev;
 *   offsets_host [G + 1] and num_spk_host [G] are host arrays, consumed before the call returns.  gamma_dev (in and out) holds
 *   the groups back to back, group g [T_g, S_g] at the double offset sum_{h<g} T_h S_h; pi_dev (in and out) group g at the
 *   offset sum_{h<g} S_h.  elbo_dev [G, max_iters], iters_dev [G].  A group with T = 0 writes only iters = 0.
 * Workspace: xv_vbx_workspace(G, offsets, num_spk, r) = 256 ceil(32 G / 256) + 8 (N (r + 2) + 3 sum_g T_g S_g) bytes, N the
 *   number of rows of the call (the group table; rho, G_t and the per-frame logsumexp; logp, lfw, lbw), is the least ws_bytes,
 *   or the code xv_vbx returns for the same groups and r; what lies beyond is not used.  ws_dev must be 8-byte aligned.
 * 1 <= S <= 64, 1 <= r <= 256, 1 <= d <= 2048, T <= 8192, anything else is XV_ERR_UNSUPPORTED.  Offsets that decrease or start
 *   below 0, ldx < d, Fa or Fb not positive (or not finite), loop_prob outside [0, 1], max_iters < 1, a NaN option, a
 *   misaligned workspace: XV_ERR_INVALID; too little workspace: XV_ERR_WORKSPACE.  Every argument check comes before the first
 *   HIP call and the outputs are untouched on any error.  num_groups = 0 returns XV_OK and touches nothing. */
int64_t xv_vbx_workspace(int64_t num_groups, const int64_t* offsets_host /* [num_groups + 1] */,
                         const int32_t* num_spk_host /* [num_groups] */, int r);
int xv_vbx(int device, const float* x_dev, int64_t ldx, const int64_t* offsets_host /* [num_groups + 1] */,
           const int32_t* num_spk_host /* [num_groups] */, int64_t num_groups, int d, const double* affine_dev /* [r, d + 1] */,
           const double* psi_dev /* [r] */, int r, double* gamma_dev /* in, out */, double* pi_dev /* in, out */, double fa,
           double fb, double loop_prob, int max_iters, double epsilon, int32_t* labels_dev /* indexed as the rows of x_dev */,
           double* elbo_dev /* [G, max_iters] */, int32_t* iters_dev /* [G] */, void* ws_dev, int64_t ws_bytes, void* stream);

/* ---- classifier-head validation loss on the GPU (csrc/loss.hip): what Trainer.valid evaluates per batch
 * (model/trainer.py:756-884), loss_i = logsumexp_c(z_ic) - z_i,label as tf.losses.sparse_softmax_cross_entropy takes it, without
 * ever writing the [n, C] logits.  Products are exact fp32 with fp32 accumulation (the tile arithmetic of the scoring calls);
 * the error bound is derived in the header of csrc/loss.hip.  No floating-point atomics: repeats are bit-identical and a
 * row's result does not depend on its position in the batch.  1 <= embed_dim <= 2048 (XV_ERR_UNSUPPORTED otherwise).
 * xv_loss_prepare_classes = `softmax/output/kernel` [embed_dim, num_classes] -> class rows [num_classes, ldc]: the transpose
 *   for XV_LOSS_SOFTMAX (tf.layers.dense, model/loss.py:30-34), with `normalize` the columns divided by
 *   sqrt(max(sum w^2, 1e-12)) (tf.nn.l2_normalize(w, dim=0), model/loss.py:133,242,328).  Once per checkpoint.
 * xv_loss_workspace = bytes of scratch xv_loss_classifier needs for n rows and num_classes classes: 256 + 16 n ceil(C / 128),
 *   against the 4 n C bytes of the logit matrix.
 * xv_loss_classifier = the four heads: XV_LOSS_SOFTMAX z = x W + b (bias_dev [num_classes] or NULL; model/loss.py:9-48);
 *   XV_LOSS_ASOFTMAX (model/loss.py:80-198; margin = m, one of 1, 2, 4, anything else XV_ERR_UNSUPPORTED as the reference
 *   raises; m = 1 is the plain cross-entropy on x W^), XV_LOSS_AMSOFTMAX (model/loss.py:201-286: phi = cos t - margin),
 *   XV_LOSS_ARCSOFTMAX (model/loss.py:289-384: phi = cos(t + margin) while cos t > cos(pi - margin), else
 *   -cos(t + margin) - 2); the target logit becomes (1 - fa) z + fa ||x|| phi with fa = 1 / (1 + lambda) from the host.
 *   Fills, per row, loss_dev, target_dev (the target logit after the margin), lse_dev and top1_dev (the class of the
 *   largest logit BEFORE the margin, the lowest index of equal ones: the argmax of model/trainer.py:1097).
 *   A label outside [0, num_classes) is never followed: the call waits for its first kernel, returns XV_ERR_INVALID and
 *   launches nothing else (this one wait makes the call unfit for hipGraph capture).  Everything after it is stream-ordered. */
enum { XV_LOSS_SOFTMAX = 0, XV_LOSS_ASOFTMAX = 1, XV_LOSS_AMSOFTMAX = 2, XV_LOSS_ARCSOFTMAX = 3 };
int xv_loss_prepare_classes(int device, const float* kernel_dev, int64_t ldk, int embed_dim, int64_t num_classes, int normalize,
                            float* classes_dev, int64_t ldc, void* stream);
int64_t xv_loss_workspace(int64_t n, int64_t num_classes);
int xv_loss_classifier(int device, const float* x_dev, int64_t ldx, int64_t n, int embed_dim, const int32_t* labels_dev,
                       const float* classes_dev, int64_t ldc, int64_t num_classes, const float* bias_dev, int head, double margin,
                       double fa, float* loss_dev, float* target_dev, float* lse_dev, int32_t* top1_dev, void* ws_dev,
                       int64_t ws_bytes, void* stream);

/* ---- loss and gradients of the classifier heads (csrc/loss_grad.hip): training a new softmax layer on a frozen encoder
 * (egs/voxceleb/v1/nnet/lib/finetune.py:6-7).  One call gives the four per-row outputs of xv_loss_classifier, bit for bit, and
 * the gradients of sum_i s loss_i with s = grad_scale (1 / n for the mean; the call never divides by n, so n = 0 is legal:
 * XV_OK, nothing touched) with respect to x, the RAW kernel and the bias.  rows_dev [num_classes, ldc] is the transpose of
 * `softmax/output/kernel`, not normalised: what xv_loss_prepare_classes(normalize = 0) writes.
 * The rule, with l the label of row i and w^_c the normalised class row (the raw row for XV_LOSS_SOFTMAX):
 *   forward  z_ic = x_i . w^_c (+ b_c), N_i = max(||x_i||, 1e-12), c_raw = z_il / N_i, c = clip(c_raw, +-(1 - 1e-12)),
 *            t_i = fs z_il + fa phi(c) N_i (fs = 1 - fa), u_ic = z_ic except u_il = t_i, p_ic = exp(u_ic - lse_i).
 *   backward sign() and the branch selectors are constants and the clip passes no derivative outside its range, as
 *            TensorFlow differentiates tf.sign, tf.where, tf.clip_by_value and tf.maximum:
 *            d_i = s (p_il - 1); G_ic = s p_ic for c != l;
 *            phi': asoftmax m = 2: 4 |c|; m = 4: sign(2 c^2 - 1) sign(c) (32 c^3 - 16 c); additive margin: 1; additive angle:
 *            sn = sqrt(max(1 - c^2, 1e-12)), dsn = -c / sn if 1 - c^2 > 1e-12 else 0, phi' = +-(cos m - dsn sin m), + while
 *            c > cos(pi - m); phi' is multiplied by [c_raw inside the clip range];
 *            G_il = d_i (fs + fa phi'), r_i = d_i fa (phi - phi' c_raw); softmax and asoftmax m = 1: G_il = d_i, r_i = 0;
 *            grad_x_i = sum_c G_ic w^_c + r_i x_i / ||x_i|| (the last term 0 when ||x_i|| <= 1e-12);
 *            gw_c = sum_i G_ic x_i; grad_bias_c = sum_i s (p_ic - [c = l_i]);
 *            softmax: grad_rows = gw.  Angular heads, q_c = sum_e w_ce^2: grad_rows_c = (gw_c - w^_c (w^_c . gw_c)) / sqrt(q_c)
 *            if q_c > 1e-12, else gw_c / 1e-6 (the floor of tf.nn.l2_normalize).
 * Outputs: loss, target, lse, top1 [n]; grad_x_dev [n, ldgx] or NULL; grad_rows_dev [num_classes, ldc] (the columns beyond
 * embed_dim are left alone); grad_bias_dev [num_classes], required when bias_dev is given.
 * Properties (tests/test_gpu_loss_grad.py): no floating-point atomics; every output is bit-identical on every repeat, for
 * every legal ws_bytes (a smaller workspace means smaller row panels; the sums over the rows run in row order whatever the
 * panel) and whatever the workspace and the outputs held before; grad_x_i and the per-row outputs do not depend on the batch
 * around row i.  The per-element error bound is derived in the header of csrc/loss_grad.hip.
 * Checks mirror xv_loss_classifier: 1 <= embed_dim <= 2048 (XV_ERR_UNSUPPORTED); a label outside [0, num_classes) gives
 * XV_ERR_INVALID after the first kernel with every output untouched (one wait: unfit for hipGraph capture).
 * Workspace, 16-byte aligned: any ws_bytes >= xv_loss_grad_workspace_min(n, C, E) is legal (XV_ERR_WORKSPACE below it):
 *   the forward workspace + C (4 round4(E) + 520) for the normalised rows, q and the bias sums + 4 E round4(C) for their
 *   transpose + 16 n + a panel of P rows of 4 (round4(C) + C + E) bytes each, P = 32.  xv_loss_grad_workspace is the size at
 *   which P reaches min(round32(n), 1024) and nothing more is used. */
int64_t xv_loss_grad_workspace(int64_t n, int64_t num_classes, int embed_dim);
int64_t xv_loss_grad_workspace_min(int64_t n, int64_t num_classes, int embed_dim);
int xv_loss_classifier_grad(int device, const float* x_dev, int64_t ldx, int64_t n, int embed_dim, const int32_t* labels_dev,
                            const float* rows_dev, int64_t ldc, int64_t num_classes, const float* bias_dev, int head, double margin,
                            double fa, double grad_scale, float* loss_dev, float* target_dev, float* lse_dev, int32_t* top1_dev,
                            float* grad_x_dev, int64_t ldgx, float* grad_rows_dev, float* grad_bias_dev, void* ws_dev,
                            int64_t ws_bytes, void* stream);

/* ---- one optimizer step on one float32 parameter tensor of `count` elements, in place (csrc/opt_step.hip): TensorFlow 1.x's
 * rules as the reference uses them (model/trainer.py:225-246, 529-533, model/loss.py:26-33), in this order, every product,
 * sum, division and square root rounded to float32 on its own (no fused multiply-add), so that numpy float32 written in the
 * same order gives the same bits (tests/helpers/ref_loss_grad.py).  l2, clip_norm, momentum and learning_rate are rounded to
 * float32 once on entry.
 *   1. g <- g + l2 * w                                  (skipped when l2 = 0; pass 0 for a bias)
 *   2. clip_norm > 0: g <- (g * clip_norm) / max(||g||, clip_norm)          (tf.clip_by_norm of this tensor alone)
 *      ||g|| = float32(sqrt(sum g^2)) with the sum in double in a fixed order, no atomics: workgroup b owns the elements
 *      [4096 b, 4096 b + 4096), thread t adds j = 4096 b + 256 i + t for i = 0 .. 15, the 64 lanes of a wave by a shuffle tree
 *      (offsets 32 .. 1), the four waves in order; then lane l adds the partials l, l + 64, ... and the same tree.
 *   3. XV_OPT_SGD:       w <- w - lr * g
 *      XV_OPT_MOMENTUM:  a <- (m * a) + g;  w <- w - lr * a;  with use_nesterov  w <- w - lr * (g + m * a)      (a: slot0)
 *      XV_OPT_ADAM:      m <- (0.9 * m) + (0.1' * g);  v <- (0.999 * v) + (0.001' * (g * g));                    (slot0, slot1)
 *                        w <- w - (lr_t * m) / (sqrt(v) + 1e-8),  lr_t = float32(lr sqrt(1 - 0.999^step) / (1 - 0.9^step)) from
 *                        double on the host, 0.1' = float32(1.0 - 0.9), 0.001' = float32(1.0 - 0.999), step counted from 1.
 * grad_dev is not written.  Unused slots may be NULL.  A non-finite or negative learning_rate, a negative l2 or clip_norm or
 * an unknown kind gives XV_ERR_INVALID before any launch.  ws_dev (8-byte aligned, xv_opt_workspace(count) bytes) is needed
 * with clip_norm > 0 only. */
enum { XV_OPT_SGD = 0, XV_OPT_MOMENTUM = 1, XV_OPT_ADAM = 2 };
int64_t xv_opt_workspace(int64_t count);
int xv_opt_step(int device, int kind, int use_nesterov, float* w_dev, const float* grad_dev, float* slot0_dev, float* slot1_dev,
                int64_t count, double learning_rate, double l2, double clip_norm, double momentum, int64_t step, void* ws_dev,
                int64_t ws_bytes, void* stream);

/* ---- one segment-level layer with its CURRENT weights, forward and backward (csrc/seg_grad.hip): what training the two dense
 * layers behind the frozen `pooling` node together with the classifier head needs (egs/voxceleb/v1/nnet/lib/finetune.py:6-7,
 * the noupdate_var_list route of model/trainer.py:309-320, 501-527).  A layer is dense + batch norm + activation
 * (model/tdnn.py:137-179): x_dev [n, in_dim] with leading dimension ldx; w_dev [out_dim, ldw] holds the ROWS of the weights, the
 * transpose of the TensorFlow `kernel` [in_dim, out_dim]; bias_dev [out_dim]; optionally gamma, beta, moving_mean and
 * moving_variance [out_dim] (all four or none: XV_ERR_INVALID otherwise), eps = 1e-3; act one of XV_SEG_ACT_*.
 * Batch norm runs in INFERENCE mode: moving_mean and moving_variance are constants, gamma and beta are trained.  The
 * reference feeds is_training = True and normalises with batch statistics; here the layers are trained on exactly the function
 * extraction and validation evaluate, and every row's result is independent of the batch around it: **parity unpinned**.
 * The rule (K = in_dim, N = out_dim; i rows, j output columns, k input columns):
 *   forward   z_ij = sum_k x_ik w_jk + b_j;  r_j = 1 / sqrt(mv_j + eps);  h_ij = gamma_j r_j (z_ij - mm_j) + beta_j (h = z
 *             without batch norm);  y_ij = act(h_ij): h, max(h, 0), or h > 0 ? h : 0.2 h (TensorFlow's leaky-ReLU slope).
 *             Writes z_dev [n, ldz], which the backward pass reads, and y_dev [n, ldy].
 *             Rounding order, every step float32: the products of z are exact fp32 on v_mfma_f32_32x32x2_f32, one fmaf chain
 *             over k ascending from 0 whose order is a function of K alone, then + b_j;  r_j = float(1 / sqrt(double(mv_j) +
 *             1e-3));  s_j = gamma_j * r_j;  d = z - mm_j;  h = fma(s_j, d, beta_j);  leaky ReLU multiplies by float(0.2).
 *   backward  given gy [n, ldgy], x, z and the parameters:  a_ij = gy_ij act'(h_ij), act' = [h > 0] for ReLU, 1 where h > 0 and
 *             0.2 elsewhere for leaky ReLU (zero belongs to the lower branch, as TensorFlow differentiates both), 1 for none;
 *             h is recomputed from z by the very instructions of the forward pass, so the mask agrees with the y written.
 *             gbeta_j = sum_i a_ij;  ggamma_j = sum_i a_ij r_j (z_ij - mm_j);  gz_ij = a_ij gamma_j r_j (gz = a without batch
 *             norm);  gbias_j = sum_i gz_ij;  gw_jk = sum_i gz_ij x_ik, rows layout [out_dim, ldw], the columns beyond in_dim
 *             left alone;  gx_ik = sum_j gz_ij w_jk [n, ldgx], or gx_dev = NULL to skip that product (the first trained layer
 *             never needs it).  ggamma_dev and gbeta_dev are written with batch norm only (and required then).
 * Properties (tests/test_gpu_seg_grad.py): no floating-point atomics; the column sums gbeta, ggamma and gbias run in double in a
 * fixed order by row index and are rounded once; the sum over the rows in gw is one fmaf chain in ascending row index whatever
 * the panel size; every output is bit-identical on every repeat, for every legal ws_bytes and whatever the workspace and the
 * outputs held before; row i of z, y and gx depends on row i and the parameters only.  The per-element error bound is derived
 * in the header of csrc/seg_grad.hip.  Both calls are stream-ordered and never wait.  n = 0 is legal: XV_OK, nothing touched.
 * 1 <= in_dim <= 16384, 1 <= out_dim <= 4096, n <= 2^24: XV_ERR_UNSUPPORTED beyond.  A leading dimension below its width, an
 * unknown activation, a missing pointer or some but not all of the four batch-norm pointers: XV_ERR_INVALID.
 * Workspace: xv_seg_forward needs none.  xv_seg_backward takes any 16-byte aligned ws_bytes >= xv_seg_workspace_min(n, in_dim,
 * out_dim) (XV_ERR_WORKSPACE below it): 1536 N for the lane sums + 4 K round4(N) for the transposed weights, each rounded up to
 * 256, + a panel of P rows of 4 (round4(N) + N + K) bytes each, P = 64.  xv_seg_workspace is the size at which P reaches
 * min(round64(n), 1024) and nothing more is used.  Both are 0 for n = 0. */
enum { XV_SEG_ACT_NONE = 0, XV_SEG_ACT_RELU = 1, XV_SEG_ACT_LRELU = 2 };
int64_t xv_seg_workspace(int64_t n, int in_dim, int out_dim);
int64_t xv_seg_workspace_min(int64_t n, int in_dim, int out_dim);
int xv_seg_forward(int device, const float* x_dev, int64_t ldx, int64_t n, int in_dim, const float* w_dev, int64_t ldw, int out_dim,
                   const float* bias_dev, const float* gamma_dev, const float* beta_dev, const float* mean_dev, const float* var_dev,
                   int act, float* z_dev, int64_t ldz, float* y_dev, int64_t ldy, void* stream);
int xv_seg_backward(int device, const float* gy_dev, int64_t ldgy, const float* x_dev, int64_t ldx, const float* z_dev, int64_t ldz,
                    int64_t n, int in_dim, const float* w_dev, int64_t ldw, int out_dim, const float* gamma_dev,
                    const float* beta_dev, const float* mean_dev, const float* var_dev, int act, float* gx_dev, int64_t ldgx,
                    float* gw_dev, float* gbias_dev, float* ggamma_dev, float* gbeta_dev, void* ws_dev, int64_t ws_bytes,
                    void* stream);

/* ---- statistics pooling of the caller's own packed rows, forward and backward (csrc/pool_grad.hip; model/pooling.py:27-52): the
 * piece between the 1-tap frame layers (tdnn4 / tdnn5; tdnn8 .. tdnn10 of the extended TDNN), which on packed frames are
 * xv_seg_forward / xv_seg_backward with one row per frame, and the segment-level layers, when both are trained behind the frozen
 * tdnn3_relu / tdnn7_relu node (tf_kaldi_speaker_amd/frame_train.py).  The pooling inside xv_forward is fused into the last
 * frozen GEMM and cannot be called on a tensor of the caller's.
 * Layout: utterance b owns the rows offsets[b] .. offsets[b + 1]) of x_dev [*, ldx], C = channels columns; offsets_dev
 *   [batch + 1] lives on the device, ascends, offsets[0] >= 0.  total_rows is a host value >= offsets[batch]; it sizes grids and
 *   nothing else.  Rows outside [offsets[0], offsets[batch]) and columns >= C are never read or written.  pooled_dev
 *   [batch, ldp] = [mean | std], 2 C wide; var_dev [batch, ldv] = the variance BEFORE the floor, C wide; gp_dev [batch, ldgp] =
 *   the gradient with respect to pooled; gx_dev [*, ldgx] has the row numbering of x.
 * Forward, per utterance of n frames and channel, every step rounded to float32 once:
 *   m = S / float(n), S = sum_t x_t (a division, not a product with a rounded reciprocal);
 *   v = Q / float(n), Q = sum_t d_t^2 with d_t = x_t - m about the COMPUTED mean, each term one fma (two sweeps, never
 *   E[x^2] - m^2);  std = sqrtf(v <= 1e-12f ? 1e-12f : v).  n = 0: m = 0, v = 0, std = sqrtf(1e-12f).
 *   Order of S and Q, a function of n alone: 16 partial sums, partial s taking the frames s, s + 16, s + 32, ... in ascending
 *   order from 0, then a binary tree over the 16, neighbours first (k = 16 in the bars of tests/helpers/ref_pool.py).
 * Backward:  live = v > 1e-12f, read from var_dev (the reference's floor mask is a constant to TensorFlow: a floored channel
 *   passes no gradient from std);  a = gm / float(n);  b = live ? gs / (float(n) * std) : 0;  d = x_t - m;  gx_t = fma(b, d, a),
 *   each operation rounded to float32 once; gm = gp[c], gs = gp[C + c].  That is gx = gm / n + gs (x - m) / (n std): the term of
 *   d var / d mean multiplies sum_t (x_t - m) = 0 and is dropped.  Nothing is written for n = 0.
 *   Per element |gx^ - gx| <= u (2 |a| + 4 |b d|)(1 + 2^-20) + 2^-149, u = 2^-24, against the float64 rule at the same float32
 *   m, std, v and gp (derived in the header of csrc/pool_grad.hip).
 * Properties (tests/test_gpu_pool_grad.py): no atomics; the outputs of an utterance are a pure function of its own rows and
 *   gradient row: the same bits on every repeat, alone or in any batch, at any position and row alignment of the packed buffer,
 *   for any total_rows, with 16-byte or 4-byte accesses, and whatever the outputs held before.  Both calls only enqueue work and
 *   never wait.
 * 1 <= channels <= 4096, total_rows <= 2^24 (and batch <= 2^24): XV_ERR_UNSUPPORTED beyond.  A leading dimension below its width
 *   (ldx, ldv, ldgx < C; ldp, ldgp < 2 C), a missing pointer, a negative batch or total_rows: XV_ERR_INVALID before any launch.
 *   batch = 0: XV_OK, nothing touched. */
int xv_stat_pool_forward(int device, const float* x_dev, int64_t ldx, int channels, const int32_t* offsets_dev, int64_t batch,
                         int64_t total_rows, float* pooled_dev, int64_t ldp, float* var_dev, int64_t ldv, void* stream);
int xv_stat_pool_backward(int device, const float* gp_dev, int64_t ldgp, const float* x_dev, int64_t ldx, int channels,
                          const int32_t* offsets_dev, int64_t batch, int64_t total_rows, const float* pooled_dev, int64_t ldp,
                          const float* var_dev, int64_t ldv, float* gx_dev, int64_t ldgx, void* stream);

/* ---- self-attentive pooling of the caller's own packed rows, forward and backward (csrc/att_pool_grad.hip; model/pooling.py:
 * 150-218): the sibling of xv_stat_pool_* for pooling_type self_attention, everything behind the key and value networks (which on
 * packed frames are xv_seg_forward / xv_seg_backward).  **Parity unpinned** against TensorFlow; pinned to torch.autograd in
 * float64 of the einsum formulation (tests/test_att_pool_host.py).
 * Layout, as xv_stat_pool_*: utterance b owns the rows offsets[b] .. offsets[b + 1]) of key_dev [*, ldk] (Dk = key_dim columns) and
 *   of value_dev [*, ldv] (Dv = value_dim columns); offsets_dev [batch + 1] is int32 on the device, ascends, offsets[0] >= 0;
 *   total_rows >= offsets[batch] is a host value that sizes grids and the workspace and nothing else.  H = heads.  query_dev
 *   [H, ldq] has dq columns, dq = Dk / H with split_key, else Dk; dv = Dv / H with split_value, else Dv.  Head h reads the key
 *   columns h dq + d when the key is split, else d, and the value columns likewise.  scale is 1 / sqrt(dq) rounded to float32 for
 *   att_use_scale, else 1.  weights_dev [*, ldw], H columns, in the row numbering of the inputs; pooled_dev [batch, ldp] = [mean |
 *   std], 2 P wide, P = H dv, column h dv + d (head-major, as combine_last_two_dimensions gives it); var_dev [batch, ldvar], P
 *   wide, the weighted variance BEFORE the floor.  gp_dev [batch, ldgp] is the gradient with respect to pooled; gkey_dev [*,
 *   ldgk], gvalue_dev [*, ldgv] have the row numbering of the inputs, gquery_dev [H, ldgq] the shape of the query.  Rows no
 *   utterance owns and columns beyond the widths are never read or written.
 * Forward, per utterance of n frames:
 *   s[t,h] = fl(scale * S), S = sum_d key q in float32: lane l of a wave one fma chain over d = l, l + 64, ... from 0, then an xor
 *   butterfly of float32 additions, distances 32 down to 1: a function of dq alone;
 *   w[t,h] = float(exp(double(s) - double(max_t s)) / Z), Z = sum_t exp(..) in double (256 interleaved partial sums in ascending
 *   frame order, then a binary tree, strides 128 down to 1), rounded to float32 ONCE;
 *   m = sum_t w v, acc = fma(w, v, acc), and var = sum_t w (v - m)^2 about the COMPUTED mean, d = fl(v - m), acc = fma(w, fl(d d),
 *   acc), both in the order of xv_stat_pool_forward: 16 partial sums, partial s the frames s, s + 16, ... ascending from 0, then
 *   the binary tree over the 16, neighbours first.  No division.  std = sqrtf(var <= 1e-12f ? 1e-12f : var).  n = 0: m = 0, var =
 *   0, std = sqrtf(1e-12f), nothing is written for rows.
 * Backward:  live = var > 1e-12f read from var_dev (the floor mask is a constant to TensorFlow); gvar = live ? fl(gs / (2 std)) :
 *   0; gm = gp[p], gs = gp[P + p].
 *   gvalue[t,(h),d] = sum_h fma(w, fma(2 gvar, fl(v - m), gm), .) from 0, heads ascending (one head when the value is split);
 *   gw[t,h] = sum_d (gm v + gvar (v - m)^2) and c[h] = sum_d (gm m + gvar var) in double, in ONE order (lane l the columns l, l +
 *   64, ..., two fmas per column, then the xor butterfly), so that they cancel bit for bit for n = 1;
 *   gscore[t,h] = float(double(w) (gw - c)), rounded once;  gkey[t,(h),d] = sum_h fma(fl(scale gscore), q, .) from 0, heads
 *   ascending (one head when the key is split);
 *   gquery[h,d] = float(double(scale) sum_b sum_t double(gscore) double(key)): per utterance the 16 partial sums and the tree of
 *   the moments in double, then the utterances in ascending order in double.  The term of d var / d m multiplies sum_t w (v - m) =
 *   0 and is dropped.  gquery of a batch without frames is 0.
 *   The per-element bound of every output is derived in the header of csrc/att_pool_grad.hip and restated in
 *   tests/helpers/ref_att_pool.py: against the float64 rule at the same float32 inputs and the float32 w, m, std, var the forward
 *   wrote.
 * Properties (tests/test_gpu_att_pool.py): no floating-point atomics; every output has the same bits on every repeat, for every
 *   legal ws_bytes, for any total_rows, for every pitch and any 4-byte aligned base (every access is a 4-byte one), and whatever
 *   the outputs and the workspace held before.  weights, pooled, var, gvalue and gkey of an utterance are a pure function of its
 *   own rows, the query and its own gradient row; gquery depends on the order of the utterances only through the order of its
 *   last sum.  Both calls only enqueue work and never wait.
 * 1 <= heads <= 16, 1 <= key_dim, value_dim <= 4096, total_rows <= 2^24, batch <= 2^20: XV_ERR_UNSUPPORTED beyond.  A split
 *   dimension that heads does not divide, a leading dimension below its width (ldp, ldgp < 2 P), a missing pointer, a negative
 *   batch or total_rows: XV_ERR_INVALID before any launch.  batch = 0: XV_OK, nothing touched.
 * Workspace of the backward (16-byte aligned; XV_ERR_WORKSPACE below the least size): c, gvar, gscore [total_rows, H], a running
 *   sum and the gquery partials of a panel of utterances; xv_att_pool_workspace_min holds one utterance per panel,
 *   xv_att_pool_workspace the whole batch, anything between is legal.  Both are 0 for batch = 0 and an xv_status for shapes the
 *   calls refuse. */
int64_t xv_att_pool_workspace(int64_t batch, int64_t total_rows, int heads, int key_dim, int value_dim, int split_key,
                              int split_value);
int64_t xv_att_pool_workspace_min(int64_t batch, int64_t total_rows, int heads, int key_dim, int value_dim, int split_key,
                                  int split_value);
int xv_att_pool_forward(int device, const float* key_dev, int64_t ldk, int key_dim, const float* value_dev, int64_t ldv, int value_dim,
                        const float* query_dev, int64_t ldq, int heads, int split_key, int split_value, float scale,
                        const int32_t* offsets_dev, int64_t batch, int64_t total_rows, float* weights_dev, int64_t ldw,
                        float* pooled_dev, int64_t ldp, float* var_dev, int64_t ldvar, void* stream);
int xv_att_pool_backward(int device, const float* gp_dev, int64_t ldgp, const float* key_dev, int64_t ldk, int key_dim,
                         const float* value_dev, int64_t ldv, int value_dim, const float* query_dev, int64_t ldq, int heads,
                         int split_key, int split_value, float scale, const int32_t* offsets_dev, int64_t batch, int64_t total_rows,
                         const float* weights_dev, int64_t ldw, const float* pooled_dev, int64_t ldp, const float* var_dev,
                         int64_t ldvar, float* gkey_dev, int64_t ldgk, float* gvalue_dev, int64_t ldgv, float* gquery_dev,
                         int64_t ldgq, void* ws_dev, int64_t ws_bytes, void* stream);

/* ---- one frame-level layer on packed utterances with its CURRENT weights, forward and backward (csrc/tconv_grad.hip): a W-tap
 * temporal convolution (tf.layers.conv2d(.., (1, W)) / tf.layers.conv1d(.., W) of model/tdnn.py: VALID, stride 1, no dilation) +
 * batch norm in INFERENCE mode + activation.  It is what training tdnn1 .. tdnn3 (tdnn1 .. tdnn7 of the extended TDNN) needs;
 * with taps = 1 it is the dense layer of xv_seg_forward / xv_seg_backward on packed frames (**parity unpinned**, as there).
 * Layout: x_dev [*, ldx] has C = channels columns; utterance b owns its rows offsets[b] .. offsets[b + 1]), n_in of them, and
 *   produces n_out = max(n_in - (W - 1), 0) output rows.  offsets_dev [batch + 1] is int32 on the device, ascends, offsets[0] >=
 *   0.  The outputs are packed densely from row 0: out_off[b] = sum_{a < b} n_out_a, computed on the device.  total_in >=
 *   offsets[batch] - offsets[0] and total_out >= out_off[batch] are host values that size grids and the workspace and nothing
 *   else.  w_dev [N = out_dim, ldw] holds the ROWS of the weights with K = W C columns, k = tau C + c: the TensorFlow kernel
 *   [W, C, N] (or [1, W, C, N]) reshaped to [W C, N] and transposed.  bias, gamma, beta, moving_mean, moving_variance [N] and act
 *   as for xv_seg_forward.
 * The rule, for output row t of utterance b (row out_off[b] + t of z, y and gy):
 *   z_tj = sum_tau sum_c x[offsets[b] + t + tau, c] w[j, tau C + c] + b_j;
 *   h, y, a = gy act'(h), gz, gbeta, ggamma and gbias are exactly the lines of xv_seg_forward / xv_seg_backward, in the same
 *   float32 rounding order (r_j = float(1 / sqrt(double(mv_j) + 1e-3)); s_j = gamma_j * r_j; d = z - mm_j; h = fma(s_j, d,
 *   beta_j); leaky ReLU multiplies by float(0.2); the backward recomputes h from the stored z by the forward's instructions);
 *   gw[j, tau C + c] = sum over all output rows of all utterances of gz_tj x[offsets[b] + t + tau, c], the columns beyond K left
 *   alone;
 *   gx[offsets[b] + s, c] = sum_tau sum_j gz_b[s - tau, j] w[j, tau C + c] over the tau with 0 <= s - tau < n_out, [*, ldgx] in the
 *   row numbering of x; every owned row is written, so an utterance with n_out = 0 gets zero rows.  gx_dev = NULL skips that
 *   product (the first layer never needs it).
 * Orders (all exact fp32 products on v_mfma_f32_32x32x2_f32, no floating-point atomics anywhere): the chain of z runs over k = tau
 *   C + c ascending from 0, then + b_j; the chain of gx over tau ascending, then j ascending (through round4(N) - N exact zeros
 *   per tap); the chain of gw over the output rows ascending, cut into S contiguous ranges of ceil32(ceil(total_out / S')) rows
 *   whose sums are added in ascending order in float32, S' = max(1, min(floor(512 / (ceil(N / 64) ceil(K / 64))), 32, ceil(total_out
 *   / 256))); the column sums gbeta, ggamma and gbias run in double over slices of max(1024, ceil64(ceil(total_out / 64))) rows,
 *   within a slice 64 interleaved partial sums in ascending row order closed by a fixed butterfly, the slices in ascending order,
 *   rounded once.  Every order is a function of the shapes and total_out alone.
 * Properties (tests/test_gpu_tconv.py): every output is bit-identical on every repeat, for every legal ws_bytes and whatever the
 *   workspace and the outputs held before; z, y and gx of an utterance are a pure function of its own rows and the parameters,
 *   alone or in any batch, at any position.  Nothing outside [offsets[0], offsets[batch]) is read; nothing outside the first
 *   total_out rows of z and y and the owned rows of gx is written.  ldx >= C is supported (the address of k is (k / C) ldx + k %
 *   C past the row's start); 16-byte accesses are used only where the bases, the leading dimensions and C allow.  The
 *   per-element error bound is derived in the header of csrc/tconv_grad.hip.  Both calls only enqueue work and never wait.
 *   batch = 0 or total_out = 0 is legal: XV_OK, nothing touched.
 * 1 <= taps <= 16, taps * channels <= 16384, 1 <= out_dim <= 4096, batch, total_in, total_out <= 2^24: XV_ERR_UNSUPPORTED
 *   beyond.  A leading dimension below its width, an unknown activation, a missing pointer, some but not all of the four
 *   batch-norm pointers, total_in < total_out in the backward call: XV_ERR_INVALID, before any launch.
 * Workspace (16-byte aligned; XV_ERR_WORKSPACE below the least size): xv_tconv_forward keeps the row maps in the first
 *   xv_tconv_forward_workspace(batch, total_out) bytes.  xv_tconv_backward takes any ws_bytes >= xv_tconv_workspace_min(..): the
 *   row maps, gz [total_out, round4(N)], the slice sums and the S planes of gw.  Nothing is panelled, so xv_tconv_workspace
 *   equals xv_tconv_workspace_min and a larger workspace is not used.  The backward call builds its own maps: it does not need
 *   the workspace of the forward call.  All three are 0 for batch = 0 or total_out = 0. */
int64_t xv_tconv_workspace(int64_t batch, int64_t total_in, int64_t total_out, int taps, int channels, int out_dim);
int64_t xv_tconv_workspace_min(int64_t batch, int64_t total_in, int64_t total_out, int taps, int channels, int out_dim);
int64_t xv_tconv_forward_workspace(int64_t batch, int64_t total_out);
int xv_tconv_forward(int device, const float* x_dev, int64_t ldx, int channels, int taps, const int32_t* offsets_dev, int64_t batch,
                     int64_t total_in, int64_t total_out, const float* w_dev, int64_t ldw, int out_dim, const float* bias_dev,
                     const float* gamma_dev, const float* beta_dev, const float* mean_dev, const float* var_dev, int act,
                     float* z_dev, int64_t ldz, float* y_dev, int64_t ldy, void* ws_dev, int64_t ws_bytes, void* stream);
int xv_tconv_backward(int device, const float* gy_dev, int64_t ldgy, const float* x_dev, int64_t ldx, int channels, int taps,
                      const int32_t* offsets_dev, int64_t batch, int64_t total_in, int64_t total_out, const float* z_dev, int64_t ldz,
                      const float* w_dev, int64_t ldw, int out_dim, const float* gamma_dev, const float* beta_dev,
                      const float* mean_dev, const float* var_dev, int act, float* gx_dev, int64_t ldgx, float* gw_dev,
                      float* gbias_dev, float* ggamma_dev, float* gbeta_dev, void* ws_dev, int64_t ws_bytes, void* stream);

/* ---- one grid convolution of the ResNet on packed utterances with its CURRENT weights, forward and backward, and the residual
 * join of a block (csrc/gconv_grad.hip): tf.layers.conv2d(.., (kh, kw), strides=(st, sf), padding='same') of model/resnet.py +
 * batch norm in INFERENCE mode + activation.  The grid twin of xv_tconv_*; it is what training conv0_1 and the blocks of the
 * ResNet-18 needs.  **Parity unpinned** against TensorFlow; pinned to torch.autograd in float64 of F.pad + F.conv2d + eval-mode
 * batch_norm + relu / leaky_relu (tests/test_gconv_host.py).
 * Layout: rows are (utterance, frame, bin).  x_dev [*, ldx] has C = channels columns; offsets_dev [batch + 1] is int32 on the
 *   device, counts FRAMES, ascends, offsets[0] >= 0; utterance b has L = offsets[b + 1] - offsets[b] frames of F_in = bins bins,
 *   its element (l, f) is row (offsets[b] + l) F_in + f.  It produces L_out = ceil(L / st) frames of F_out = ceil(F_in / sf) bins
 *   (TensorFlow's 'same'); along each axis pad = max((out - 1) s + k - in, 0) / 2 zeros stand in front (integer division), taken
 *   per utterance along time and independently along frequency.  The outputs are packed densely from frame 0: out_off[b] = sum_{a
 *   < b} L_out_a, computed on the device; element (lo, fo) is row (out_off[b] + lo) F_out + fo of z, y and gy.  total_in >=
 *   offsets[batch] - offsets[0] and total_out >= out_off[batch] are host values in FRAMES that size grids and the workspace and
 *   nothing else.  w_dev [N = out_dim, ldw] holds the ROWS of the weights with K = kh kw C columns, k = (dl kw + df) C + c: the
 *   HWIO kernel [kh, kw, C, N] reshaped to [kh kw C, N] and transposed.  bias_dev may be NULL (the ResNet's grid convolutions
 *   have use_bias=False), and then gbias_dev may be NULL too; gamma, beta, moving_mean, moving_variance [N] and act as for
 *   xv_seg_forward.
 * The rule, with X the gathered view: X[o, (dl kw + df) C + c] = x at (lo st - pad_t + dl, fo sf - pad_f + df, c) of the
 *   utterance of output row o, a ZERO where that frame lies outside the utterance's own L frames or the bin outside [0, F_in):
 *   z_oj = sum_k X[o, k] w[j, k] (+ b_j);
 *   h, y, a = gy act'(h), gz, gbeta, ggamma and gbias are exactly the lines of xv_tconv_forward / xv_tconv_backward;
 *   gw[j, k] = sum over all output rows of all utterances of gz_oj X[o, k], the columns beyond K left alone;
 *   gx[i, c] = sum over the taps (dl, df) ascending, then j ascending, of gz[o(i, tap), j] w[j, tap C + c] in the row numbering
 *   of x [*, ldgx]: for input element (l, f) a tap contributes only where l + pad_t - dl is divisible by st and f + pad_f - df by
 *   sf and the quotients are an output position of the same utterance.  Every owned input row is written; an input that no
 *   output reads (odd positions under a strided 1 x 1) gets exact zeros.  gx_dev = NULL skips that product.
 * Orders (all exact fp32 products on v_mfma_f32_32x32x2_f32, no floating-point atomics anywhere): the chain of z runs over k
 *   ascending from 0, then + b_j; the chain of gx over the taps ascending, then j ascending (through round4(N) - N exact zeros per
 *   tap, and through the taps that contribute nothing as zero operands); the chain of gw over the output rows ascending, cut into
 *   S contiguous ranges of ceil32(ceil(rows_out / S')) rows whose sums are added in ascending order in float32, S' = max(1,
 *   min(ceil(1024 / (ceil(N / 64) ceil(K / 64))), 256, ceil(rows_out / 1024))), rows_out = total_out F_out; the column sums
 *   gbeta, ggamma and gbias run in double in the slice order of xv_tconv_backward over the rows_out rows.  Every order is a
 *   function of the shapes and total_out alone.
 * Properties (tests/test_gpu_gconv.py): every output is bit-identical on every repeat, for every legal ws_bytes and whatever the
 *   workspace and the outputs held before; z, y and gx of an utterance are a pure function of its own rows and the parameters,
 *   alone or in any batch, at any position.  Nothing outside the owned rows is read; nothing outside the first total_out F_out
 *   rows of z and y and the owned rows of gx is written.  ldx >= C is supported; 16-byte accesses are used only where the bases,
 *   the leading dimensions and C allow.  The per-element error bound is derived in the header of csrc/gconv_grad.hip.  Both
 *   calls only enqueue work and never wait.  batch = 0 or total_out = 0 is legal: XV_OK, nothing touched.
 * kh, kw in {1, 3}, st, sf in {1, 2}, kh kw channels <= 16384, 1 <= out_dim <= 4096, 1 <= bins <= 4096, batch <= 2^24, total_in
 *   bins and total_out F_out <= 2^24 rows: XV_ERR_UNSUPPORTED beyond.  A leading dimension below its width, an unknown activation,
 *   a missing pointer, some but not all of the four batch-norm pointers: XV_ERR_INVALID.  Every check comes before the first
 *   launch: a refused call writes nothing.
 * Workspace (16-byte aligned; XV_ERR_WORKSPACE below the least size): xv_gconv_forward keeps out_off and the map of the output
 *   rows in the first xv_gconv_forward_workspace(batch, total_out, bins, sf) bytes.  xv_gconv_backward takes any ws_bytes >=
 *   xv_gconv_workspace_min(..): the two row maps, gz [rows_out, round4(N)], the slice sums and the S planes of gw.  Nothing is
 *   panelled, so xv_gconv_workspace equals xv_gconv_workspace_min and a larger workspace is not used.  The backward call builds
 *   its own maps.  All three are 0 for batch = 0 or total_out = 0, and XV_ERR_UNSUPPORTED for a window or stride the calls refuse.
 * The residual join, on [rows, N = out_dim] operands each with a pitch of its own, every access a scalar float32 one:
 *   xv_add_act_forward:  s = p + q (one float32 addition), y = act(s) by the activation's line of xv_seg_forward;
 *   xv_add_act_backward: g = gy act'(s), s recomputed by the forward's instruction, act'(0) that of the lower branch; g is the
 *   gradient of both p and q.  The outputs are the bits of numpy float32 written the same way.  rows <= 2^28, out_dim <= 65536:
 *   XV_ERR_UNSUPPORTED beyond; rows = 0: XV_OK, nothing touched. */
int64_t xv_gconv_workspace(int64_t batch, int64_t total_in, int64_t total_out, int bins, int kh, int kw, int st, int sf, int channels,
                           int out_dim);
int64_t xv_gconv_workspace_min(int64_t batch, int64_t total_in, int64_t total_out, int bins, int kh, int kw, int st, int sf,
                               int channels, int out_dim);
int64_t xv_gconv_forward_workspace(int64_t batch, int64_t total_out, int bins, int sf);
int xv_gconv_forward(int device, const float* x_dev, int64_t ldx, int channels, int bins, int kh, int kw, int st, int sf,
                     const int32_t* offsets_dev, int64_t batch, int64_t total_in, int64_t total_out, const float* w_dev, int64_t ldw,
                     int out_dim, const float* bias_dev, const float* gamma_dev, const float* beta_dev, const float* mean_dev,
                     const float* var_dev, int act, float* z_dev, int64_t ldz, float* y_dev, int64_t ldy, void* ws_dev,
                     int64_t ws_bytes, void* stream);
int xv_gconv_backward(int device, const float* gy_dev, int64_t ldgy, const float* x_dev, int64_t ldx, int channels, int bins, int kh,
                      int kw, int st, int sf, const int32_t* offsets_dev, int64_t batch, int64_t total_in, int64_t total_out,
                      const float* z_dev, int64_t ldz, const float* w_dev, int64_t ldw, int out_dim, const float* gamma_dev,
                      const float* beta_dev, const float* mean_dev, const float* var_dev, int act, float* gx_dev, int64_t ldgx,
                      float* gw_dev, float* gbias_dev, float* ggamma_dev, float* gbeta_dev, void* ws_dev, int64_t ws_bytes,
                      void* stream);
int xv_add_act_forward(int device, const float* p_dev, int64_t ldp, const float* q_dev, int64_t ldq, int64_t rows, int out_dim, int act,
                       float* y_dev, int64_t ldy, void* stream);
int xv_add_act_backward(int device, const float* gy_dev, int64_t ldgy, const float* p_dev, int64_t ldp, const float* q_dev, int64_t ldq,
                        int64_t rows, int out_dim, int act, float* g_dev, int64_t ldg, void* stream);

/* ---- batch norm in TRAINING mode behind the stored product z of a trained layer (csrc/bn_batch.hip): the batch statistics, h
 * and y, the moving-average update (tf.layers.batch_normalization(training=True) with the UPDATE_OPS of model/trainer.py:501-527)
 * and the gradient through the statistics.  z_dev [n, ldz] (N = out_dim columns) is what xv_seg_forward / xv_tconv_forward store
 * when they are called without batch norm and with XV_SEG_ACT_NONE.  The backward produces no gbias, gw or gx: the caller hands
 * gz as gy to xv_seg_backward / xv_tconv_backward, called with the four batch-norm pointers null and XV_SEG_ACT_NONE, whose mask
 * kernels pass it through (gbias_j = sum_i gz_ij, gw and gx by their own rules).
 * **Parity unpinned** against TensorFlow's own kernels (none at hand); pinned instead to torch.nn.functional.batch_norm(training
 *   =True, eps=1e-3) in float64, forward, autograd and running statistics (tests/test_bn_batch_host.py).
 * Forward (float32 in and out; gamma, beta [N]; act one of XV_SEG_ACT_*; every step behind v is a line of csrc/layer_lines.h):
 *   S1_j = sum_i double(z_ij),  mu_j = float(S1_j / n);   S2_j = sum_i (double(z_ij) - double(mu_j))^2,  v_j = float(S2_j / n)
 *   (two sweeps, the second about the rounded mean; the biased variance);
 *   r_j = float(1 / sqrt(double(v_j) + 1e-3)),  s_j = gamma_j * r_j,  h_ij = fma(s_j, z_ij - mu_j, beta_j),  y_ij = act(h_ij)
 *   -> y_dev [n, ldy], batch_mean_dev [N] = mu, batch_var_dev [N] = v.
 *   d = float(1.0 - momentum),  f = float(double(n) / double(max(n - 1, 1))),  v'_j = bessel ? v_j * f : v_j;
 *   moving_mean_j     <- moving_mean_j     - (moving_mean_j     - mu_j) * d
 *   moving_variance_j <- moving_variance_j - (moving_variance_j - v'_j) * d      in place, each operation rounded to float32 on
 *   its own (tf assign_moving_average, zero_debias off).  moving_mean_dev and moving_var_dev: both or neither.
 *   bessel: tf.layers.batch_normalization takes the fused kernel for a rank-4 input, and the fused kernel hands the moving
 *   variance the Bessel-corrected batch variance (n / (n - 1)); a rank-2 or rank-3 input takes tf.nn.moments and the biased one.
 *   The normalisation itself uses the biased variance either way.  The caller knows the rank (tf_kaldi_speaker_amd.tail_train).
 * Backward (gy_dev [n, ldgy]; batch_mean_dev and batch_var_dev as the forward returned them):
 *   h as in the forward (the same bits),  a_ij = gy_ij act'(h_ij),  xh_ij = double(r_j) * (double(z_ij) - double(mu_j)),
 *   A_j = sum_i double(a_ij),  G_j = sum_i double(a_ij) * xh_ij,  gbeta_j = float(A_j),  ggamma_j = float(G_j),
 *   gz_ij = float(double(s_j) * (double(a_ij) - A_j / n - xh_ij * G_j / n))       (one rounding, from the unrounded sums)
 *   -> gz_dev [n, ldgz], ggamma_dev [N], gbeta_dev [N].
 * Order of every column sum (that of xv_tconv_backward's): slices of max(1024, ceil64(ceil(n / 64))) rows, within a slice 64
 *   interleaved partial sums (lane l takes the rows i = l mod 64, ascending) closed by a fixed butterfly, the slices in ascending
 *   order in double, rounded once.  A function of n alone; no floating-point atomics.
 * Properties (tests/test_gpu_bn_batch.py): every output is bit-identical on every repeat, for every legal ws_bytes and whatever
 *   the workspace and the outputs held before.  Every access is a scalar float32 one, so any 4-byte aligned pointer and any
 *   leading dimension >= out_dim give the bits of the contiguous layout.  The per-element error bound is derived in the header of
 *   csrc/bn_batch.hip (r amplifies the error of v where v is far below 1e-3 or comparable to it; the bound carries |dr/dv|).
 *   Both calls only enqueue work and never wait.
 * 1 <= out_dim <= 4096, n <= 2^24: XV_ERR_UNSUPPORTED beyond.  n < 1, out_dim < 1, a leading dimension below out_dim, momentum
 *   outside [0, 1] or NaN, an unknown activation, a missing pointer, one moving vector without the other: XV_ERR_INVALID.  Every
 *   check comes before the first launch: a refused call writes nothing.
 * Workspace (16-byte aligned; XV_ERR_WORKSPACE below the least size): the slice sums and the unrounded column sums, 32 N slices +
 *   16 N bytes, each rounded up to 256.  Nothing is panelled, so xv_bn_batch_workspace equals xv_bn_batch_workspace_min and a
 *   larger workspace is not used.  Both are 0 for n < 1 or out_dim < 1. */
int64_t xv_bn_batch_workspace(int64_t n, int out_dim);
int64_t xv_bn_batch_workspace_min(int64_t n, int out_dim);
int xv_bn_batch_forward(int device, const float* z_dev, int64_t ldz, int64_t n, int out_dim, const float* gamma_dev,
                        const float* beta_dev, int act, double momentum, int bessel, float* moving_mean_dev, float* moving_var_dev,
                        float* y_dev, int64_t ldy, float* batch_mean_dev, float* batch_var_dev, void* ws_dev, int64_t ws_bytes,
                        void* stream);
int xv_bn_batch_backward(int device, const float* gy_dev, int64_t ldgy, const float* z_dev, int64_t ldz, int64_t n, int out_dim,
                         const float* batch_mean_dev, const float* batch_var_dev, const float* gamma_dev, const float* beta_dev,
                         int act, float* gz_dev, int64_t ldgz, float* ggamma_dev, float* gbeta_dev, void* ws_dev, int64_t ws_bytes,
                         void* stream);

/* ---- metric-learning loss heads on the GPU (csrc/metric_loss.hip): what validation needs for a checkpoint trained with
 * `semihard_triplet_loss` (model/loss.py:387-527) or `angular_triplet_loss` (:530-663; validated with `e2e_valid_loss`,
 * :666-734, model/trainer.py:424-427).  Pinned to the reference's float64 numpy twins (model/test_utils.py:21-86, 118-154,
 * 694-857) through tests/golden/metric_*.npz.  Everything is double, from float32 rows.
 * A group is one batch: rows x_1 .. x_B of length d, labels l_1 .. l_B (any int32 values).
 *   u_i = x_i s_i, s_i = 1 / sqrt(max(sum_t x_it^2, 1e-12)) (l2_scaling, model/common.py:45-58); G(a, b) = sum_t a_t b_t,
 *   a pure function of the VALUES of the two rows (not of their position, tile or group).
 * XV_METRIC_SEMIHARD: v = u with `normalize`, else x.  n_i = G(v_i, v_i), D2(i, j) = max(n_i - 2 G(v_i, v_j) + n_j, 0),
 *   d = D2 with `squared`, else sqrt(D2); d(i, i) = 0.  For every ordered pair (i, j), j != i, l_j == l_i, over the negatives k
 *   (l_k != l_i): z = the least d(i, k) > d(i, j) (strict), or the largest d(i, k) if there is none; the term is
 *   max(margin + d(i, j) - z, 0).  loss = sum / max(pairs, 1e-16).  An anchor without a negative contributes nothing.
 * XV_METRIC_ANGULAR_ALL / _HARD: c(i, j) = clip(G(u_i, u_j), -1, 1); pos(c) by pos_head: XV_LOSS_ASOFTMAX margin = m: c
 *   (m = 1), 2 sign(c) c^2 - 1 (m = 2), s3 (8 c^4 - 8 c^2 + 1) + s4 with s0 = sign(c), s3 = sign(2 c^2 - 1) s0,
 *   s4 = 2 s0 + s3 - 3 (m = 4; sign(0) = 0; any other m is XV_ERR_UNSUPPORTED); XV_LOSS_AMSOFTMAX: c - margin;
 *   XV_LOSS_ARCSOFTMAX: t = c cos(margin) - sqrt(1 - c^2) sin(margin), -t - 2 when c <= cos(pi - margin), else t.
 *   ALL: over anchors i, positives j != i and negatives k, t = c(i, k) - pos(c(i, j)); S = sum max(t, 0), A = #{t > 1e-12},
 *   V = the number of triplets; loss = S / (A + 1e-16).  HARD: hp_i = min of pos(c(i, j)) over l_j == l_i (j = i included),
 *   hn_i = max of c(i, k) over the negatives, row = max(hn_i - hp_i, 0), 0 without a negative; loss = the mean over the B rows.
 * XV_METRIC_GE2E_SOFTMAX / _CONTRASTIVE: classes = the distinct labels in order of first appearance; s_c = the sum of u_i over
 *   the class in row order; chat_c = unit(s_c), e_i = unit(s_c(i) - u_i) (unit = the scaling above: a class of one row has
 *   e_i = 0); sim(i, c) = G(u_i, chat_c), sim(i, c(i)) = G(u_i, e_i); z = w sim + b.  SOFTMAX: row = lse(z_i) - z_i,c(i)
 *   (max-shifted), top1_i = the label of the arg-max class, the earliest class among equals.  CONTRASTIVE: row =
 *   1 - sigma(z_i,c(i)) + max(0, max_{c != c(i)} sigma(z_ic)), sigma from exp(-|z|).  loss = the mean over the rows.
 *   e2e_valid_loss is SOFTMAX with w = 20, b = 0.
 * Layout: group g owns the rows offsets[g] .. offsets[g + 1]) of x_dev [*, ldx]; labels_dev and the three row outputs are
 *   indexed by the same row numbers (total = offsets[G]); offsets_host is a host array, consumed before the call returns.
 *   row_loss_dev = the anchor's un-normalised sum (the row's loss for HARD and GE2E); row_count_dev = the anchor's positive
 *   pairs (SEMIHARD), its active triplets (ALL), 1 otherwise; row_top1_dev (GE2E; may be NULL).  group_loss_dev [G] = the
 *   sequential double sum of the group's row_loss in row order, normalised as above; group_count_dev [G, 2] = (pairs, 0),
 *   (A, V), (B, 0), (B, rows whose top1 is their own label).
 *   A group's outputs are a pure function of its own rows, labels and the options: the same bits on every repeat, alone or in
 *   any batch, in any group order, for every legal ws_bytes.  No floating-point atomics.
 * Workspace: xv_metric_loss_workspace is the least ws_bytes (tables, three doubles per row and, for groups over 1024 rows or
 *   the GE2E kinds, one slot of 128 (B | 1) resp. 8 B (d + B) bytes rounded up to 256, B = the largest group); every further slot lets
 *   one more workgroup run at a time (up to 1024); xv_metric_loss_slot_bytes is the size of one (0: the kind needs none for
 *   groups of max_rows rows).  Both return XV_ERR_INVALID for arguments xv_metric_loss refuses.
 *   ws_dev must be 8-byte aligned.
 * 1 <= d <= 4096, 1 .. 4096 rows per group, ascending offsets from >= 0, ldx >= d, a known kind (and pos_head for the angular
 *   kinds), finite margin, w, b: XV_ERR_INVALID otherwise; too little workspace: XV_ERR_WORKSPACE.  Every argument check comes
 *   before the first HIP call and the outputs are untouched on any error.  num_groups = 0 returns XV_OK and touches nothing. */
enum { XV_METRIC_SEMIHARD = 0, XV_METRIC_ANGULAR_ALL = 1, XV_METRIC_ANGULAR_HARD = 2, XV_METRIC_GE2E_SOFTMAX = 3,
       XV_METRIC_GE2E_CONTRASTIVE = 4 };
int64_t xv_metric_loss_workspace(int64_t num_groups, const int64_t* offsets_host /* [num_groups + 1] */, int d, int kind);
int64_t xv_metric_loss_slot_bytes(int max_rows, int d, int kind);
int xv_metric_loss(int device, const float* x_dev, int64_t ldx, const int64_t* offsets_host /* [num_groups + 1] */,
                   int64_t num_groups, int d, const int32_t* labels_dev, int kind,
                   int pos_head /* XV_LOSS_ASOFTMAX | _AMSOFTMAX | _ARCSOFTMAX, angular kinds */, double margin, int squared,
                   int normalize, double w, double b, double* row_loss_dev /* [total] */, int64_t* row_count_dev /* [total] */,
                   int32_t* row_top1_dev /* [total] or NULL */, double* group_loss_dev /* [G] */,
                   int64_t* group_count_dev /* [G, 2] */, void* ws_dev, int64_t ws_bytes, void* stream);

/* ---- gradients of the triplet heads (csrc/metric_loss_grad.hip): what fine-tuning with `semihard_triplet_loss` or
 * `angular_triplet_loss` needs (egs/voxceleb/v1/nnet/lib/finetune.py, model/trainer.py:113-129).  Notation, layout and forward
 * outputs are those of xv_metric_loss above: row_loss, row_count, group_loss and group_count are bit for bit what it writes for
 * the same arguments (one product chain, one mining order).  grad_x_dev [total, ldg] = float32(grad_scale dL_g / dx_i), L_g the
 * loss of the row's group; everything before that rounding is double.  The gradient is that of model/loss.py:387-663 as
 * TensorFlow differentiates it wherever TensorFlow's choice is unique: **parity unpinned** against TensorFlow, pinned to
 * torch.autograd in float64 (tests/test_metric_grad_host.py).  Comparisons, masks, counts and the normalisers (pairs, A + 1e-16,
 * B) are constants.  The choices:
 *   Hinge: max(t, 0) passes 1 iff t > 0; so does the clamp of D2 (it passes iff D2 > 0).
 *   Selections (the semi-hard negative z, hp_i and hn_i of HARD) send their gradient to one element, the lowest column among
 *     equals.  TensorFlow splits a tie evenly: different on exact ties only.
 *   XV_METRIC_SEMIHARD: an active term of the pair (i, j) adds +1 at d(i, j) and -1 at d(i, k*).  dd/dD2 = 1 with `squared`,
 *     else 1 / (2 d) where D2 > 0 and 0 where D2 == 0 (the reference's mask * 1e-16, model/common.py:86-92: duplicate rows give
 *     0, never inf).  n_i = G(v_i, v_i) is differentiated: dD2/dv_i = 2 (v_i - v_j).
 *   XV_METRIC_ANGULAR_ALL: every triplet with t > 0 adds +1 at c(i, k) and -pos'(c(i, j)) at c(i, j).
 *   XV_METRIC_ANGULAR_HARD: a row with a negative and hn_i - hp_i > 0 adds +1/B at c(i, k*) and -pos'(c(i, j*)) / B at c(i, j*).
 *     The pair (i, i) carries no gradient: c(i, i) is the constant 1 (TensorFlow would form inf * 0 there for arcsoftmax).
 *   pos': asoftmax 1 (m = 1), 4 |c| (m = 2), s3 (32 c^3 - 16 c) (m = 4), signs being constants; amsoftmax 1; arcsoftmax
 *     cos m + c sin m / sqrt(1 - c^2), negated on the branch c <= cos(pi - m).
 *   Clip: dc/dG = 1 for -1 < G < 1, else 0; pos' is never evaluated at |c| = 1.
 *   Normalisation (`normalize`, always for the angular kinds): gx_i = s_i (gu_i - (gu_i . u_i) u_i) where sum x^2 > 1e-12
 *     (tested as s_i < 1e6), else s_i gu_i: the max branch is a constant.
 *   No NaN or inf comes out of finite rows whose products stay finite.
 * A group's outputs are a pure function of its own rows, labels and the options: the same bits on every repeat, alone or in any
 *   batch, in any group order, for every legal ws_bytes, leading dimension and 4-byte aligned base, whatever the buffers held
 *   before.  No floating-point atomics.  The columns d .. ldg - 1 of grad_x_dev are never written.  The per-element error bound
 *   is derived in the header of csrc/metric_loss_grad.hip (tests/helpers/ref_metric_grad.bounds()).
 * Kinds 0 .. 2 only: the GE2E kinds return XV_ERR_UNSUPPORTED (the reference never trains with them), as does a group over
 *   1024 rows (panel and counts of a group live in LDS).  ldg >= d and a finite grad_scale, else XV_ERR_INVALID; everything
 *   xv_metric_loss refuses is refused alike.  Every argument check comes before the first HIP call and the outputs are untouched
 *   on any error.  num_groups = 0 returns XV_OK and touches nothing.
 * Workspace (8-byte aligned): xv_metric_loss_grad_workspace is the least ws_bytes: tables, three doubles per row and one slot of
 *   8 B (B + d) bytes rounded up to 256, B = the largest group (dL/dM [B, B] and its product with the rows [B, d]); every
 *   further slot lets one more group run at a time (up to 64).  It returns the negative code for arguments the call refuses. */
int64_t xv_metric_loss_grad_workspace(int64_t num_groups, const int64_t* offsets_host /* [num_groups + 1] */, int d, int kind);
int xv_metric_loss_grad(int device, const float* x_dev, int64_t ldx, const int64_t* offsets_host /* [num_groups + 1] */,
                        int64_t num_groups, int d, const int32_t* labels_dev, int kind, int pos_head, double margin, int squared,
                        int normalize, double grad_scale, double* row_loss_dev /* [total] */, int64_t* row_count_dev /* [total] */,
                        double* group_loss_dev /* [G] */, int64_t* group_count_dev /* [G, 2] */,
                        float* grad_x_dev /* [total, ldg] */, int64_t ldg, void* ws_dev, int64_t ws_bytes, void* stream);

/* ---- back-end training statistics on the GPU (csrc/backend.hip): the sums behind `ivector-mean`, `ivector-compute-lda` and
 * `ivector-compute-plda` (egs/voxceleb/v1/run.sh:384-400, egs/sre/v1/run.sh:399-411); the d x d linear algebra behind them is
 * host float64 (tf_kaldi_speaker_amd.backend).  Kaldi is absent from the reference tree: **parity unpinned**.
 * xv_gram_f64 = G = sum_r w_r (x_r - c)(x_r - c)^T: x_dev [n, ldx] float32, c_dev [d] double or NULL (0), w_dev [n] double or
 *   NULL (1), g_dev [d, d] double, both triangles written, G == G^T bitwise.  x - c is evaluated in double (one rounding), w is
 *   applied to one operand, products and sums are double (v_mfma_f64_16x16x4_f64): with y = x - c in double,
 *   |G - sum_r w_r y_ri y_rj| <= (n + 16) 2^-53 sum_r |w_r y_ri y_rj|.  No floating-point atomics: repeated calls are
 *   bit-identical.  n = 0 writes zeros.  1 <= d <= 2048 (XV_ERR_UNSUPPORTED otherwise); ws_dev is a scratch buffer of at least
 *   xv_gram_f64_workspace(n, d) bytes (XV_ERR_WORKSPACE when ws_bytes is less; the size depends on (n, d) alone and may be 0,
 *   then ws_dev may be NULL).  Every argument check comes before the first HIP call.
 * xv_gram_f64_rows64 = the same over double rows (the class means of xv_class_mean_f64: the between-class scatter).
 * xv_class_mean_f64 = per-class means in double, the index convention of xv_speaker_mean: class s owns the rows
 *   utt_index[spk_offsets[s] .. spk_offsets[s+1]) of x_dev [n, ldx]; out[s] = (their sum in double, in that order) / count,
 *   minus c_dev [dim] when it is not NULL; a class without rows gets zeros; a row number outside [0, n) is never followed
 *   (the class gets NaN; the caller checks its indices on the host). */
int64_t xv_gram_f64_workspace(int64_t n, int d);
int xv_gram_f64(int device, const float* x_dev, int64_t ldx, int64_t n, int d, const double* c_dev, const double* w_dev,
                double* g_dev, void* ws_dev, int64_t ws_bytes, void* stream);
int xv_gram_f64_rows64(int device, const double* x_dev, int64_t ldx, int64_t n, int d, const double* c_dev, const double* w_dev,
                       double* g_dev, void* ws_dev, int64_t ws_bytes, void* stream);
int xv_class_mean_f64(int device, const float* x_dev, int64_t ldx, int64_t n, int dim, const int32_t* spk_offsets_dev,
                      const int32_t* utt_index_dev, int64_t num_classes, const double* c_dev, double* out_dev, int64_t ldo,
                      void* stream);

/* ---- score calibration and fusion on the GPU (csrc/calibrate.hip): the statistics of a prior-weighted logistic regression
 * over a trial list, and the affine fusion it fits.  The reference has no such step (its only fusion is the equal-weight mean
 * of misc/utils/average_score.py): **parity unpinned**; tests/helpers/ref_calibration.py restates the rules below in numpy.
 * A trial i has k scores s_i1 .. s_ik (1 <= k <= XV_LOGREG_MAX_SYSTEMS, XV_ERR_UNSUPPORTED otherwise), row i of scores_dev
 * [n, lds] float32 with lds >= k (the columns k .. lds - 1 are never read), and a flag targets_dev[i] (uint8, non-zero: target).
 * theta_host = (w_1 .. w_k, b), host doubles.  llr_i = ((w_1 s_i1 + w_2 s_i2) + ...) + b in double, ascending k, the bias last,
 * every product and sum rounded on its own (no fused multiply-add), so that numpy written in this order gives the same bits.
 * xv_score_fuse = out_dev[i] = (float)llr_i, one rounding.  n = 0 touches nothing.
 * xv_logreg_stats = one pass over the trials.  With z_i = llr_i + tau, softplus(x) = max(x, 0) + log1p(exp(-|x|)), sigma
 *   evaluated from exp(-|z|) (no overflow for either sign), c_i = c_tar, x_i = -z_i, r_i = -sigma(-z_i) for a target and
 *   c_i = c_non, x_i = z_i, r_i = sigma(z_i) otherwise, and a_i = (s_i1, .., s_ik, 1):
 *     stats_dev[0]                F = sum_i c_i softplus(x_i)
 *     stats_dev[1 .. k + 1]       g = sum_i c_i r_i a_i
 *     stats_dev[k + 2 ..]         the upper triangle of H = sum_i c_i sigma(z_i) sigma(-z_i) a_i a_i^T, row by row
 *                                 ((0,0) .. (0,k), (1,1) .. (k,k)): 1 + (k + 1) + (k + 1)(k + 2) / 2 doubles in all;
 *     counts_dev[0 .. 2]          targets, non-targets, and rows with a score that is not finite: such a row is counted here
 *                                 and left out of everything else, the class counts included;
 *     counts_dev[3 + j], [11 + j] for threshold j < num_thresholds <= XV_LOGREG_MAX_THRESHOLDS (thresholds_host, doubles):
 *                                 #{target: (float)llr_i < eta_j} and #{non-target: (float)llr_i >= eta_j}, compared in double;
 *                                 0 for j >= num_thresholds.  19 int64 in all.
 *   c_tar = pi / N_tar, c_non = (1 - pi) / N_non and tau = log(pi / (1 - pi)) make F the objective of the calibration at prior
 *   pi; k = 1, theta = (1, 0), tau = 0 and c = 1 / (2 N) give Cllr ln 2.  The caller passes the weights (it knows the class
 *   counts), which keeps one set of sums.  All sums are double; no atomics, neither floating-point nor integer: a workgroup
 *   owns 16384 consecutive rows, adds them in a fixed order and a second launch adds the workgroups' partials in a fixed order,
 *   so the result is a pure function of (scores, targets, the host arguments): every repeat, every workspace at or above
 *   xv_logreg_workspace(n, k) bytes (XV_ERR_WORKSPACE below it; 0 for n = 0, then ws_dev may be NULL) and whatever lies
 *   behind row n give the same bits.  |entry - exact sum| is far below 1e-12 sum_i |term_i| (a term is a handful of
 *   roundings; a sum is at most 64 serial additions and a tree).  n = 0 writes zeros.  n < 0, n >= 2^40, lds < k, a null
 *   pointer or num_thresholds outside 0..8 is XV_ERR_INVALID; every argument check comes before the first HIP call, and
 *   everything is stream-ordered: the call never waits for the device. */
#define XV_LOGREG_MAX_SYSTEMS 8
#define XV_LOGREG_MAX_THRESHOLDS 8
int64_t xv_logreg_workspace(int64_t n, int k);
int xv_logreg_stats(int device, const float* scores_dev, int64_t lds, int64_t n, int k, const uint8_t* targets_dev,
                    const double* theta_host, double tau, double c_tar, double c_non, const double* thresholds_host,
                    int num_thresholds, double* stats_dev, int64_t* counts_dev, void* ws_dev, int64_t ws_bytes, void* stream);
int xv_score_fuse(int device, const float* scores_dev, int64_t lds, int64_t n, int k, const double* theta_host, float* out_dev,
                  void* stream);

/* ---- reverberation and additive noise (csrc/reverb.hip) ------------------------------------------------------------
 * What Kaldi's wav-reverberate does to one utterance, on a packed batch: the stage-2 augmentation of egs/sre/v1/run.sh and
 * egs/voxceleb/v2/run_aug.sh, whose wav.scp lines are `wav-reverberate ... |` pipelines.  Kaldi is not in the reference tree:
 * **parity unpinned**; the rule restates wav-reverberate.cc as published and is the specification
 * (tests/helpers/ref_reverb.py states it in float64 numpy).
 *
 * An utterance has int16 samples x[0..N), N >= 1, at sample rate fs; optionally an impulse response h[0..L) = int16 / 32768
 * (exact in float32), 1 <= L <= 65536; J >= 0 additive signals v_j[0..M_j) with snr_j in dB, a start time t_j in seconds and
 * an extended length M'_j >= 1 (M'_j = M_j unless the signal came from a nested --duration pipe).  All rates are equal.
 *   1. P_before = (sum x^2) / N.
 *   2. With an RIR: y[n] = sum_k h[k] x[n - k] for n in [0, N + L - 1).  p = the lowest index of the largest *signed* h
 *      (Vector::Max).  b = trunc(0.001 fs), a = trunc(0.05 fs); the early window is [s, e) = [max(0, p - b), min(L, p + a));
 *      E = sum_n e[n]^2 / (N + (e - s) - 1), e = the same convolution restricted to the taps in [s, e).
 *      Without an RIR: y = x, E = P_before, p = 0.  Y = len(y).
 *   3. For j in order: P_j = sum_{i < M'_j} v_j[i mod M_j]^2 / M'_j, g_j = sqrt(10^(-snr_j / 10) E / P_j),
 *      o_j = trunc(t_j fs); for 0 <= i < min(M'_j, Y - o_j): y[o_j + i] += g_j v_j[i mod M_j].  P_j = 0 is an error of that
 *      utterance (status 1); no inf is ever written.
 *   4. P_after = sum y^2 / Y.
 *   5. scale = volume if volume > 0; else sqrt(P_before / P_after) if normalize_output (P_after = 0: status 2); else 1.
 *   6. shift = p if there is an RIR and shift_output, else 0.  n_out = trunc(duration fs) if duration > 0, else N if
 *      shift_output, else Y.  out[i] = scale y[(i + shift) mod Y] for i < n_out: the plain range when n_out <= N, the full
 *      tail when shift_output = false, and the repetition that fills a --duration longer than the signal.
 *   7. int16 output: trunc toward zero, then saturation to [-32768, 32767]; the saturated samples are counted per utterance.
 *   8. Sums of squares and every scalar (E, P_*, g_j, scale) are double; partial sums are added in a fixed order, one per
 *      workgroup, then a second fixed-order pass; no floating-point atomics.  y is float32.  An utterance's outputs are a
 *      pure function of its own inputs: the same bits on every repeat, alone or in any batch, and for every workspace of at
 *      least xv_reverb_workspace bytes.
 * The float32 output stays within scale eps[n] + |ref| delta of the rule in exact arithmetic; csrc/reverb.hip derives
 * eps and delta.
 *
 * Tables are host arrays.  waves_dev / rirs_dev / noises_dev are packed int16 device buffers of wave_samples / rir_samples /
 * noise_samples samples; several utterances may name the same impulse response or additive signal.  Utterance i reads
 * waves[wave_off .. + wave_len) and writes out[out_off .. + out_len), out_len = n_out of rule 6; both sets of offsets rise
 * without overlap.  rir_len = 0: no RIR.  Its additive signals are the rows [noise_begin, + noise_count) of the noise table
 * (rising).  out_i16_dev or out_f32_dev may be NULL, not both; an utterance whose status_dev is not 0 gets zeros.
 * peak_dev[i] = p, clipped_dev[i] = the saturated samples of the int16 output (0 without one).  xv_reverb validates every
 * table before the first HIP call (XV_ERR_INVALID: offsets that do not rise or leave a buffer, a length outside [1, 2^31),
 * N + L - 1 or n_out at or above 2^31, out_len other than n_out, fs outside [100, 1e6], snr outside [-200, 200] dB, a negative
 * start time, volume above 1e6; XV_ERR_UNSUPPORTED: L > 65536; XV_ERR_WORKSPACE: ws_bytes below xv_reverb_workspace) and only
 * enqueues on `stream`.  xv_reverb_workspace makes the same checks and returns the bytes or the negative code.
 * xv_reverb_tile: the convolution's tile of outputs per workgroup and chunk of taps per LDS pass (tests size shapes by them). */
#define XV_REVERB_TILE 2048
#define XV_REVERB_CHUNK 256
#define XV_REVERB_MAX_TAPS 65536
typedef struct {
  int64_t wave_off, wave_len;         /* N */
  int64_t rir_off, rir_len;           /* L; 0: none */
  int64_t noise_begin, noise_count;   /* J rows of the noise table */
  int64_t out_off, out_len;           /* n_out */
  double sample_rate, duration, volume;
  int32_t shift_output, normalize_output;
} xv_reverb_utt;
typedef struct {
  int64_t off, len, ext_len;          /* M, M' */
  double snr_db, start_time;
} xv_reverb_noise;
int xv_reverb_tile(int* tile, int* chunk);
int64_t xv_reverb_workspace(const xv_reverb_utt* utts_host, int64_t num_utts, const xv_reverb_noise* noises_host,
                            int64_t num_noises, int64_t wave_samples, int64_t rir_samples, int64_t noise_samples,
                            int64_t out_samples);
int xv_reverb(int device, const int16_t* waves_dev, int64_t wave_samples, const int16_t* rirs_dev, int64_t rir_samples,
              const int16_t* noises_dev, int64_t noise_samples, const xv_reverb_utt* utts_host, int64_t num_utts,
              const xv_reverb_noise* noises_host, int64_t num_noises, int16_t* out_i16_dev, float* out_f32_dev,
              int64_t out_samples, int32_t* status_dev, int32_t* peak_dev, int32_t* clipped_dev, void* ws_dev, int64_t ws_bytes,
              void* stream);

/* ---- host-side ark I/O (csrc/ark_io.cpp; no HIP calls, usable without a GPU) ---------------------
 * Batch counterpart of dataset/kaldi_io.py read_mat_ark (:974-994, records per _read_mat_binary
 * :1014-1031 / _read_compressed_mat :1071-1115) and write_vec_flt (:915-946): the extraction driver
 * (extract.py:64,93) reads and writes one record per Python call; these parse / format a whole batch. */
typedef struct xv_ark_reader xv_ark_reader;
/* Open a binary matrix ark by path, or wrap an already open descriptor (path == NULL; e.g. the read
 * end of a `cmd |` rspecifier pipe).  The descriptor is closed by xv_ark_close only when opened here. */
int xv_ark_open(const char* path, int fd, xv_ark_reader** out);
/* Open a Kaldi script file (`key rxfilename` lines, rxfilename = `file` or `file:offset`; what
 * dataset/kaldi_io.py read_mat_scp :953-972 walks one record per call, and what `scp:${sdata}/feats.scp` means
 * to the Kaldi binaries of run_extract_embeddings.sh:47).  Records are reached by seeking; consecutive
 * entries of one ark are read through one descriptor.  XV_ERR_UNSUPPORTED for ranges / pipes in the table.
 * xv_ark_next_batch then delivers the table's records in table order.  Float-vector records ('FV ', 'DV ';
 * e.g. vad.scp) are delivered as [dim, 1] matrices by both readers. */
int xv_ark_open_scp(const char* scp_path, xv_ark_reader** out);
int64_t xv_ark_scp_count(const xv_ark_reader* r);
/* rows / cols of every record of the table (headers only: one seek + one short read per record; the
 * utterance lengths the sharder needs, utils/split_data.sh's role in run_extract_embeddings.sh:43).  Rewinds. */
int xv_ark_scp_shapes(xv_ark_reader* r, int32_t* rows, int32_t* cols, int64_t capacity);
/* Read consecutive utterances ('FM ', 'DM ', 'CM ' records) until `max_frames` frames or `max_utts`
 * utterances are collected or the next one does not fit.  Utterances with fewer than `min_frames` rows
 * are dropped and counted (extract.py:65-67).  dst: float32 [frames, dim] row-major, utterance i =
 * rows offsets[i]..offsets[i+1]; keys: '\n'-terminated keys back to back.  Returns the number of
 * utterances (0 = end of stream) or a negative status code; the message is xv_ark_error(r). */
int xv_ark_next_batch(xv_ark_reader* r, int64_t max_frames, int max_utts, int min_frames, float* dst,
                      int64_t dst_capacity, int32_t* offsets, char* keys, int64_t keys_capacity, int* n_utts,
                      int* dim);
/* Shape of the record whose header has been parsed but not delivered (after xv_ark_next_batch failed with
 * "a single utterance does not fit ..."): lets the caller retry with a larger buffer.  XV_ERR_STATE if none. */
int xv_ark_pending_shape(const xv_ark_reader* r, int32_t* rows, int32_t* cols);
int64_t xv_ark_skipped(const xv_ark_reader* r);
/* Threads that copy the float payloads of a batch when the ark is a regular file opened by name (the file is mapped for
 * header parsing and the payloads are pread() straight into `dst`).  Default: 4 on hosts with >= 8 cores, else 2 / 1.
 * n is clamped to [1, 16].  No reference counterpart (dataset/kaldi_io.py reads one record at a time). */
int xv_ark_set_copy_threads(xv_ark_reader* r, int n);
const char* xv_ark_error(const xv_ark_reader* r);
void xv_ark_close(xv_ark_reader* r);
/* Format n float vectors (row i = data + i*ld, `dim` values) as binary Kaldi vector records
 * "key SP \0B FV \4 <i32 dim> payload" into `out`; returns the byte count or a negative xv_status. */
int64_t xv_ark_format_vectors(const char* keys, int n, const float* data, int dim, int64_t ld, char* out,
                              int64_t out_capacity);

/* Copy n blocks (src[i], nbytes[i] bytes) back to back into dst with up to `threads` threads: the staging copy of a ragged batch
 * that arrives as separate [T_i, d] matrices (Trainer.predict, model/trainer.py:886-913, called once per utterance by
 * extract.py:89; here once per batch).  Returns the number of bytes copied or a negative xv_status. */
int64_t xv_pack_rows(const void* const* src, const int64_t* nbytes, int n, void* dst, int threads);

/* CRC-32C (Castagnoli) of n bytes continuing from `crc` (0 to start): the checksum of TensorFlow checkpoint-V2 index blocks and
 * tensors (the weight source of model/trainer.py:277-295; tf-kaldi-speaker_amd/tf_checkpoint.py applies the LevelDB mask). */
uint32_t xv_crc32c(uint32_t crc, const void* data, int64_t n);

/* ---- training input: stage the bytes of a planned batch, decode them on the device (csrc/train_stage.cpp, csrc/train_batch.hip) ----
 * A training batch is B chunks of `length` frames, chunk i being rows [start_i, start_i + length) of one archive record (what
 * dataset/data_loader.py's workers cut out of dataset/kaldi_io.py:1118-1171 _read_compressed_submat).  The stager copies only
 * the bytes those rows need into one caller-provided (pinned) buffer and describes them; the decode turns the staged bytes
 * into the packed float32 batch [B * length, dim] the trainers take.  The host does no arithmetic on the features.
 *
 * One descriptor per chunk.  The staged payload of chunk i starts at byte payload_off (a multiple of 16) of the staged buffer:
 *   XV_TRAIN_FM  rows x cols float32, row-major;   XV_TRAIN_DM  rows x cols float64, row-major;
 *   XV_TRAIN_CM  cols x rows bytes, COLUMN-major (Kaldi's kOneByteWithColHeaders payload, cut to the staged rows), and at byte
 *                header_off (a multiple of 8) the cols per-column headers of four uint16 each; gmin / grange are the record's
 *                global header.
 * `rows` is the staged row count and first_row the staged row that is frame 0 of the chunk (the stager stages exactly the
 * chunk: first_row = 0, rows = length).  Output row i * length + t, column c < dim, is element (first_row + t, c):
 *   FM: the float as it is.   DM: (float)value, one rounding.
 *   CM: the rule of csrc/ark_io.cpp (Kaldi's CompressedMatrix), all in double, each operation rounded on its own:
 *       p_k = (double)(float)(gmin + grange * 1.52590218966964e-05 * h_k), k = 0..3 (h the column's header);  v the byte;
 *       x = p0 + (p1 - p0) / 64 * v          for v <= 64
 *           p1 + (p2 - p1) / 128 * (v - 64)  for v <= 192
 *           p2 + (p3 - p2) / 63 * (v - 192)  else;            out = (float)x, one rounding.
 *     The device code is compiled without fused contraction and uses IEEE division, so every element has the bits
 *     xv_ark_next_batch gives for the same record.
 * Columns dim .. ld of the output are not written.  xv_train_batch_decode checks every descriptor on the host before the first
 * HIP call (XV_ERR_INVALID: an unknown kind, payload_off not a multiple of 16 or header_off of 8, cols < 1, dim > cols or
 * dim < 1, length < 1, first_row < 0, first_row + length > rows, a payload or header that reaches past staged_bytes, ld < dim,
 * num_chunks < 1, num_chunks * ceil(length / 64) * ceil(dim / 64) >= 2^31, a null pointer; XV_ERR_WORKSPACE: ws_bytes below
 * xv_train_batch_workspace), copies the descriptors into ws_dev in stream order and launches once: it never waits for the
 * device, and the descriptor array may be reused as soon as it returns.
 *
 * xv_train_stage: rxfiles holds n '\n'-terminated rxfilenames `file` or `file:offset` (feats.scp's), the offset pointing at
 * the record's "\0B" (a key in front of it is skipped); chunk i is rows [starts[i], starts[i] + length) of record i.  It reads
 * each record's header, lays the payloads out in chunk order at 16-byte boundaries (for CM the column headers first) and fills
 * chunks[i]; the layout depends on the records alone, never on `threads` (clamped to [1, 16]; they only pread).  A chunk that
 * cannot be staged (a pipe or a range as rxfilename, a file that cannot be opened, a truncated record, an unknown kind, a
 * record of fewer than starts[i] + length rows) gets status[i] = XV_ERR_INVALID (XV_ERR_UNSUPPORTED for pipes and ranges),
 * kind 0 and no bytes; the message of the first such chunk goes to err (NUL-terminated).  *staged_bytes is the byte count of
 * the layout.  Returns the number of chunks that were not staged, XV_ERR_WORKSPACE when dst_capacity is below *staged_bytes
 * (nothing is copied then), or XV_ERR_INVALID for bad arguments. */
#define XV_TRAIN_FM 1
#define XV_TRAIN_DM 2
#define XV_TRAIN_CM 3
typedef struct {
  int64_t payload_off, header_off;
  int32_t kind, cols, rows, first_row;
  float gmin, grange;
} xv_train_chunk;
int64_t xv_train_batch_workspace(int64_t num_chunks);
int xv_train_batch_decode(int device, const void* staged_dev, int64_t staged_bytes, const xv_train_chunk* chunks_host,
                          int64_t num_chunks, int length, int dim, float* out_dev, int64_t ld, void* ws_dev, int64_t ws_bytes,
                          void* stream);
int xv_train_stage(const char* rxfiles, int n, const int32_t* starts, int length, int threads, void* dst, int64_t dst_capacity,
                   xv_train_chunk* chunks, int32_t* status, int64_t* staged_bytes, char* err, int64_t err_capacity);

/* Trainer.close (model/trainer.py:270-275). */
void xv_destroy(xv_handle* h);

const char* xv_last_error(const xv_handle* h);

#ifdef __cplusplus
}
#endif
#endif /* XVEC_HIP_H_ */
