// Internal model of the C-ABI layer (api_*.hip): the handle with its graph of layers, ops, values and nodes, and the batch
// plan with its steps.  Shared helpers live in xv::api; nothing here is exported from the shared library.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/xvec_hip.h"
#include "xv_kernels.h"

namespace xv {
namespace api {

constexpr int kSlackRows = 512;        // readable rows after every activation buffer (GEMM tile / conv window overreach)
constexpr int kAlign = 256;

struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  hipError_t alloc(size_t n) {
    release();
    bytes = n;
    if (n == 0) return hipSuccess;
    return hipMalloc(&p, n);
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
  }
};

struct DeviceGuard {   // leave the caller's current device untouched
  int prev = -1;
  bool ok = true;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) { ok = false; return; }
    if (prev != dev && hipSetDevice(dev) != hipSuccess) ok = false;
  }
  ~DeviceGuard() {
    int cur = -1;
    if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
  }
};

// ------------------------------------------------------------------------------ graph
enum Stage : int { ST_AFFINE = 0, ST_BN = 1, ST_ACT = 2 };

struct HostTensor {
  std::vector<int64_t> shape;
  std::vector<float> data;
  bool set = false;
};

// An affine layer: temporal convolution (w > 1) or dense (w == 1), optional BN, optional activation.
struct Layer {
  std::string kernel_name, bias_name, bn_scope, alpha_name;
  std::string ep[3];          // endpoint key per stage ("" when the stage does not exist)
  int w = 1, cin = 0, cout = 0;
  bool has_bn = false;
  int act = ACT_NONE;         // activation of the final stage
  // device
  DevBuf wt;                  // fp32 [Npad][Kpad]                      (fp32 MFMA kernel)
  DevBuf wfr;                 // same values, MFMA-fragment-major: [Npad/32][Kpad/32][plane*2+channel tile][64 lanes][16 B]
  DevBuf wsb;                 // split-blocked bf16 hi/lo [Npad][Kpad/32][128 B] (bf16x3 kernel)
  bool use_split = false;     // this layer runs on the bf16x3 kernel
  bool im2col = false;        // first layer in a split mode: its input is the caller's fp32 feature matrix, staged per forward
  int cin_pad = 0;            // > 0: staged as SB rows of cin_pad (= cin rounded up to 32) channels per frame and convolved
                              // like any other w-tap layer (slab reuse across the taps); 0 with im2col: rows materialised
  // ResNet 2-D convolutions on the zero-bordered grid (csrc/grid.hip): 0 = 1-D conv / dense,
  // 1 = 3x3 'same' stride (1,sw), 2 = 1x1 shortcut stride (1,sw), 3 = conv5 (1 x Fin, valid), 4 = conv0 (cin 1)
  int mode = 0;
  int Fin = 0, Fout = 0, sw = 1;
  int st = 1;                 // stride along time of a grid convolution (2: first block of stages 2-4 under resnet_time_stride)
  bool has_bias = true;
  int K() const { return mode == 1 ? 9 * cin : (mode == 3 ? Fin * cin : (mode == 4 ? 9 : w * cin)); }
  DevBuf vec;                 // [bias | bn_scale | bn_shift | alpha | ones] each cout floats
  int in_exp = 0, out_exp = 0; // fp16 split formats: the split copy of the input / output holds value * 2^exp (act_exponent below)
  bool use_f6 = false;        // XV_PREC_F16F6: this multi-tap convolution runs on gemm_f16f6_kernel (input converted to its block format)
  DevBuf wf6m, wf6x;          // its weights: f16 main fragments [N/32][cin/32][8 taps][2][64 lanes][16 B]; fp6 cross operands (gemm_f16f6.hip)
  DevBuf wdir;                // conv0 (mode 4): fp32 [9][cout] kernel, then bn_scale[cout], bn_shift[cout] (direct kernel, csrc/grid.hip)
  int Kpad = 0, Npad = 0;
  int final_stage() const { return act != ACT_NONE ? ST_ACT : (has_bn ? ST_BN : ST_AFFINE); }
  const float* d_bias() const { return static_cast<const float*>(vec.p); }
  const float* d_scale() const { return d_bias() + cout; }
  const float* d_shift() const { return d_bias() + 2 * cout; }
  const float* d_alpha() const { return alpha_name.empty() ? nullptr : d_bias() + 3 * cout; }
  const float* d_ones() const { return d_bias() + 4 * cout; }
};

enum OpKind : int {
  OP_GEMM = 0,        // layer
  OP_STAT_POOL,       // statistics pooling
  OP_ATT_SCORES,      // key . query
  OP_ATT_SOFTMAX,     // in place on the scores buffer (modelled as its own value)
  OP_ATT_POOL,        // weighted mean/std
  OP_AFFINE_ACT,      // att_post_bn / att_post_relu
  OP_L2_SCALE,        // endpoints["output"] with feature_norm
  OP_GRID_MAXPOOL     // 3x3 'same' max-pool on a grid value (resnet_maxpooling)
};

// A value is a matrix produced by an op (or the network input, value 0).
struct Value {
  int grid_F = 0;     // > 0: zero-bordered grid value with grid_F frequency bins (rows = (F0+2B)*grid_S)
  int grid_S = 0;     // its pitch: positions per padded time row (csrc/grid.hip: F + 1, or F + 2 under a stride-2 reader)
  bool frame_level = true;
  int ctx = 0;        // temporal context consumed (frame-level values): rows = F[tlevel] - B*ctx
  int tlevel = 0;     // time resolution: utterance b has ceil(L_b / 2^tlevel) frames (resnet_time_stride; else 0)
  int cols = 0;
  int sb_exp = 0;     // fp16 split formats: the split-blocked copy of this value holds value * 2^sb_exp
};

struct Op {
  int kind = OP_GEMM;
  int layer = -1;     // OP_GEMM
  int in0 = -1, in1 = -1;   // value ids
  int out = -1;       // value id
};

struct Node {         // an endpoints[...] key
  std::string name;
  int op = -1;        // producing op
  int stage = -1;     // OP_GEMM: stage to emit; OP_AFFINE_ACT: 1 = bn only, 2 = bn + act
  bool att_weights = false;
};

}  // namespace api
}  // namespace xv

struct xv_handle {
  xv_model_desc desc{};
  int device = 0;
  bool finalized = false;
  std::string err;
  std::mutex mu;                                      // graph / weights / options
  std::mutex err_mu;                                  // h->err (any thread may fail)
  std::mutex prof_mu;                                 // profiling records (xv_forward from several threads)
  // options (xv_set_option)
  int opt_pool_fusion = 1;                            // statistics pooling fused into the last frame layer's epilogue
  int opt_tail_split = 1;                             // K-split of the last, nearly empty round of GEMM tiles
  int opt_grid_f6 = 1;                                // XV_PREC_F16F6: the stride-1 3 x 3 ResNet convolutions of >= 128 channels on the two-unit kernel
  int opt_slab3 = 1;                                  // one-tap GEMM layers on the three-slab-buffer kernel
  int opt_first_walk = 1;                             // staged first layer (<= 5 taps) on the walking-workgroup kernel (gemm_first.hip):
                                                      // 1 = as the producer of the two-unit block format, 2 = every shape it takes, 0 = never
  int opt_grid_compact = 1;                           // ResNet grid convolutions enumerate output bins only (split precisions)
  int opt_att_fusion = 1;                             // attention scores / weighted moments in the GEMM epilogues
  int opt_profile_dominant = 0;                       // xv_profile_*: bracket only the step with the most FLOPs of a plan
  // device index arrays of destroyed plans, kept for the next plan (no hipMalloc / hipFree per ragged batch)
  std::mutex pool_mu;
  std::vector<xv::api::DevBuf> pool;
  size_t pool_bytes = 0;
  std::map<std::string, xv::api::HostTensor> tensors; // expected variables
  std::vector<xv::api::Layer> layers;
  std::vector<xv::api::Value> values;
  std::vector<xv::api::Op> ops;
  std::vector<xv::api::Node> nodes;
  // attention extras
  xv::api::DevBuf query;        // [H, dk_h]
  xv::api::DevBuf ovf_flag;     // fp16 split formats, kFlagBufWords ints (xv_kernels.h): [0] set by any kernel that converted a value beyond
                                // the fp16 range; [1] bits of the largest feature magnitude staged since the last reset (underflow guard);
                                // then the staging kernels' per-wave and per-utterance maxima
  xv::api::DevBuf query_eff;    // [H, Npad of the last key layer]: the query of head h over the padded key width, zero
                                // outside the head's slice (fused score epilogue)
  int key_npad = 0;
  int att_dk_h = 0, att_dk = 0, att_dv = 0;
  int final_ctx = 14;           // temporal context of the pooled frames (tdnn 14, etdnn 22)
  std::string post_bn_scope, post_alpha_name;
  xv::api::DevBuf post_vec;     // [scale | shift | alpha] each pool_dim floats
  int pool_dim = 0;
  // optional per-op event profiling (xv_profile_begin / xv_profile_end)
  struct ProfRec { hipEvent_t e0, e1; const xv_plan* plan; int step; };
  bool profiling = false;
  std::vector<hipEvent_t> prof_pool;
  size_t prof_next = 0;
  std::vector<ProfRec> prof_recs;
  int prof_forwards = 0;
};

namespace xv {
namespace api {

// How the rows of a GEMM step are enumerated (api_plan.hip decides, and builds the row map of that form).
enum GemmForm : int {
  FORM_ROWS = 0,      // 1-D convolution / dense layer: one row per output frame
  FORM_TROWS,         // two-unit form of a stride-1 3 x 3 grid convolution: GEMM rows = padded time rows x frequency bins
  FORM_COMPACT,       // grid convolution whose GEMM rows are the output bins only (csrc/grid.hip, compact form)
  FORM_GRID,          // grid convolution over every input position (time stride 1 or 2)
  FORM_CONV5,         // 1 x Fin valid convolution: one row per padded time row
  FORM_CONV0          // first ResNet convolution: one row per output grid position
};

struct PlanStep {
  int op = -1;
  int stage = -1;               // stage override for the target op, else the op's final stage
  bool to_out = false;          // writes the user's output buffer
  int64_t out_off = -1;         // workspace byte offset of the fp32 output (-1: none / user buffer)
  int64_t out_sb_off = -1;      // workspace byte offset of the split-blocked output (-1: none)
  int64_t in0_off = -1, in1_off = -1;   // fp32 inputs; -2 = network input
  int64_t in0_sb_off = -1;      // split-blocked input
  int64_t rows_in = 0, rows_out = 0;
  int M = 0;                    // GEMM rows to compute
  int form = FORM_ROWS;         // GEMM: how those rows are enumerated (GemmForm)
  bool trows() const { return form == FORM_TROWS; }
  bool compact() const { return form == FORM_COMPACT; }
  int rowmap = -1;              // index into plan rowmaps (conv layers)
  int64_t scratch_off = -1;     // per-step scratch (im2col rows / split-K partials), released after the step
  int64_t scratch2_off = -1;    // two-unit layers: the K-split partials of the tail tiles (scratch_off holds the converted input)
  int ksplit = 1;               // split-K slices of a small-M fp32 GEMM, or of the tail M tiles of a bf16x3 GEMM
  int tail_mt = 0;              // bf16x3: M tiles computed K-split (gemm_bf16x3_tail_plan)
  bool fuse_pool = false;       // GEMM: emit pooling partials instead of activations; STAT_POOL: finalize only
  int lvl_in = 0, lvl_out = 0;  // time level of the input / output value
  int64_t frames_out = 0;       // total frames of the batch at the output's time level
  bool grid_cover = false;      // grid-valued output whose border is re-zeroed by zero-writing GEMM rows (no memset)
  bool out_f6 = false;          // XV_PREC_F16F6: this layer writes its split-blocked output in the block format of gemm_f16f6.hip ...
  bool in_f6 = false;           // ... because its only reader is this kind of layer, which then needs no conversion pass
  int arow = -1;                // compact: index into plan rowmaps of the window positions (GemmArgs::arow)
  int fuse_att = 0;             // GEMM: 1 = score partials instead of the key, 2 = weighted moments instead of the value;
                                // ATT_SCORES / ATT_SOFTMAX / ATT_POOL: 1 = the fused form of that op
  int64_t att_w_off = -1;       // fuse_att 2: workspace offset of the softmax output (weights [rows, H])
  int64_t att_s0_off = -1;      // workspace offset of the per-slot weight sums [pool_slots, H]
  int64_t att_ld = 0;           // fuse_att 1: row stride of the partial-score planes
  bool unpad_to_out = false;    // grid-valued target node: GEMM writes the padded grid, then it is unpadded into `out`
  int64_t flops = 0, bytes = 0;
};

}  // namespace api
}  // namespace xv

struct xv_plan {
  xv_handle* h = nullptr;
  xv_plan_info info{};
  std::vector<int32_t> offsets_slotbase;
  xv::api::DevBuf d_offsets;        // [B+1]
  std::vector<int32_t> lvl_offsets[4];   // host copies of the frame offsets per time level (the async uploads read them); levels > 0 only under resnet_time_stride
  xv::api::DevBuf d_lvl[4];         // device copies of levels 1..3 ([0] unused: level 0 is d_offsets)
  const int32_t* dev_offsets(int level) const {
    return static_cast<const int32_t*>(level > 0 ? d_lvl[level].p : d_offsets.p);
  }
  xv::api::DevBuf d_rowmaps;        // concatenated row maps
  std::vector<int64_t> rowmap_off;  // element offsets into d_rowmaps
  std::vector<xv::api::PlanStep> steps;
  xv::api::DevBuf d_row2utt;        // fused pooling: utterance of each pooled row
  xv::api::DevBuf d_slotbase;       // fused pooling: [B] slot base per utterance
  int64_t pool_slots = 0;
  int dominant_step = 0;            // index of the step with the most algorithmic FLOPs
};

namespace xv {
namespace api {

// Record a failure on the handle (and for xv_last_error(NULL)) and return `code`.  Defined in api_graph.hip.
int fail(xv_handle* h, int code, const char* fmt, ...);

#define XV_HIP(h, expr)                                                                              \
  do {                                                                                               \
    hipError_t _e = (expr);                                                                          \
    if (_e != hipSuccess)                                                                            \
      return fail((h), XV_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__,  \
                  __LINE__);                                                                         \
  } while (0)

inline int64_t align_up(int64_t v, int64_t a) { return (v + a - 1) / a * a; }

inline int act_of(const xv_model_desc& d) {
  return d.relu_type == XV_ACT_PRELU ? ACT_PRELU : (d.relu_type == XV_ACT_LRELU ? ACT_LRELU : ACT_RELU);
}

// Fl[k] = total frames of the batch at time level k (Fl[0] = frame_offsets[B])
inline int64_t value_rows(const xv_handle* h, int vid, const int64_t* Fl, int B) {
  const Value& v = h->values[vid];
  if (v.grid_F > 0) return (Fl[v.tlevel] + 2 * (int64_t)B) * v.grid_S;
  return v.frame_level ? Fl[v.tlevel] - (int64_t)B * v.ctx : B;
}

inline int64_t value_bytes(const xv_handle* h, int vid, const int64_t* Fl, int B) {
  const Value& v = h->values[vid];
  return align_up((value_rows(h, vid, Fl, B) + kSlackRows) * (int64_t)v.cols * 4, kAlign);
}

inline int sb_ld(int cols) { return (int)align_up(cols, 32); }

inline int64_t value_sb_bytes(const xv_handle* h, int vid, const int64_t* Fl, int B) {
  const Value& v = h->values[vid];
  return align_up((value_rows(h, vid, Fl, B) + kSlackRows) * (int64_t)sb_ld(v.cols) * 4, kAlign);
}

}  // namespace api
}  // namespace xv
