// Internal launch interface between the C-ABI layer (api_*.hip) and the gfx950 kernels.
// Host-side structs only; nothing here is exported from the shared library.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/xvec_hip.h"

namespace xv {

// Epilogue activation applied after  v = acc * scale[n] + shift[n].
enum Act : int { ACT_NONE = 0, ACT_RELU = 1, ACT_LRELU = 2, ACT_PRELU = 3, ACT_TANH = 4 };

constexpr float kLreluAlpha = 0.2f;       // tf.nn.leaky_relu default (model/tdnn.py:33)
// fp16 range guard buffer of a handle: kFlagWords ints ([0] overflow flag, [1] bits of a feature maximum carried over, [2..3] scratch
// of xv_flags_async, [kUttSmallWord] bits of the largest |feature| of an utterance that stayed below 2^-8, 0 = none), then
// kFeatMaxSlots floats: the largest feature magnitude each wave of the feature staging kernel saw since the last read-out, then
// kUttMaxSlots words: the bits of the largest |feature| of utterance b of the forward being staged (feat_stage_sb_kernel; folded into
// the flag words and cleared again by feat_utt_fold_kernel inside the same step: zero between forwards, never read out)
constexpr int kFlagWords = 8, kUttSmallWord = 4, kFeatMaxSlots = 32768;      // 8192 workgroups x 4 waves
constexpr int kUttMaxSlots = 32768;
constexpr int kFlagBufWords = kFlagWords + kFeatMaxSlots + kUttMaxSlots;
constexpr float kVarFloor = 1e-12f;       // VAR2STD_EPSILON (model/pooling.py:6)

// One "overlapping-row" GEMM:  Y[rowmap[m], n] = act((sum_k A[m,k] * Wt[n,k]) * scale[n] + shift[n])
//   A[m,k] = X[(m + k / cin) * ldx + k % cin]      (== X[m*ldx + k] when ldx == cin)
// A dense layer has K == cin; a temporal convolution of width w has K == w*cin, so that row m
// of A is the w consecutive input frames starting at frame m (model/tdnn.py:42-47).
struct GemmArgs {
  const float* X;         // activations, fp32
  int64_t ldx;            // row stride of X in elements
  int cin;                // channels per input frame
  int M;                  // rows of A to compute (input rows minus w-1)
  int K;                  // w * cin
  int N;                  // output channels
  const float* Wt;        // packed weights [Npad][Kpad], k contiguous, zero padded
  int Kpad;               // multiple of 32
  int Npad;               // multiple of 128
  const float* scale;     // [N]
  const float* shift;     // [N]
  const float* alpha;     // [N] PReLU slopes (ACT_PRELU) or nullptr
  int act;
  const int32_t* rowmap;  // [M] output row or -1 (skip); nullptr = identity
  float* Y;               // fp32 output (may be nullptr when only the split planes are wanted)
  int64_t ldy;
  // bf16x3 path: activations consumed by a split GEMM are carried in the split-blocked (SB)
  // format of xv_common.h (per row: blocks of [32 x bf16 hi | 32 x bf16 lo], 128 bytes).
  const void* Xsb;        // SB input (bf16x3 kernel), row stride ldsbx elements (x4 bytes)
  int64_t ldsbx;          // multiple of 32; == cin for convolutions
  void* Ysb;              // SB output or nullptr
  int ldsb;               // channels per SB output row incl. zero padding (multiple of 32)
  const void* Wsb;        // packed weights in SB format [Npad][Kpad/32][128 bytes]
  const void* Wfr = nullptr;   // weights, MFMA-fragment-major (gemm_bf16x3_wreg_kernel)
  const void* Wx6 = nullptr;   // XV_PREC_F16F6 layers: block-scaled fp6 cross-term weights (gemm_f16f6.hip; Wfr then holds the f16 main weights)
  int ysb_f6 = 0;              // gemm_f16f6 kernel: write Ysb in ITS activation block format (f16 hi | fp6 hi / lo codes | scales) -- the
                               // consumer is another two-unit layer and no conversion pass is needed
  int slab3 = 1;               // one-tap layers: three slab buffers / slabs two steps ahead (gemm_bf16x3_w1p3_kernel); 0 = the
                               // two-buffer kernel (same arithmetic, bit-identical results; xv_set_option "slab3")
  int* ovf = nullptr;          // f16 only: set to 1 when a value beyond the fp16 range was converted (checked by the host)
  int nbin = 0;                // gemm_f6v2_kernel, ResNet form: frequency bins per time row (a second tile dimension), and the byte
  int64_t bin_x_bytes = 0;     // offset of a bin's windows inside a row of A; bin b writes output rows rowmap[m] + b
  float sb_mul = 1.f;          // fp16 split formats: the split-blocked / fp6-block output holds y * sb_mul, a per-layer power of two that
                               // keeps the activations' low halves normal (|y * sb_mul| ~ 2^4 rms; the reader's per-channel scale
                               // carries 1 / sb_mul exactly: api_weights.hip, act_exponent).  The fp32 output Y is never scaled.
  int f16 = 0;                 // split format of both operands: 0 = bf16 hi/lo (bf16x3), 1 = fp16 hi/lo (f16x3: same layout and
                               // MFMA rate, 11 + 11 significand bits instead of 8 + 8; values beyond +-65504 overflow)
  long long* trace = nullptr;  // debug: per-workgroup phase timestamps (XVEC_TRACE_K), 4 per workgroup
  // split-K (fp32 kernel, small-M layers that gemm_f32_seg_kernel does not take): slice s of `ksplit` accumulates K tiles
  // [s*kper, (s+1)*kper) and writes RAW accumulators to partial[s][M][Npad]; a reduce kernel
  // sums the slices in order (deterministic) and applies the epilogue.
  int ksplit;             // 0/1 = off
  int raw;                // epilogue: store acc unchanged (scale 1, shift 0, no activation)
  float* partial;         // [ksplit][M][Npad] fp32 workspace (bf16x3 tail form: [ksplit][tail_mt * 128][Npad])
  int tail_mt = 0;        // bf16x3 kernel: the last `tail_mt` M tiles are computed K-split in `ksplit` slices (see
                          // gemm_bf16x3_tail_plan) and finished by a reduce kernel
  // fused statistics pooling (dense layer feeding statistics_pooling, model/pooling.py:27-52):
  // instead of storing the activations, every 64-row wave tile writes, per channel and per
  // utterance segment inside the tile, sum(x) and sum((x - segment mean)^2) to
  //   pool_part[(slot * 2 + {0,1}) * N + n],  slot = pool_slotbase[b] + (row >> 6)
  // (each slot is written exactly once -> deterministic); launch_pool_finalize merges the slots.
  float* pool_part;
  const int32_t* pool_row2utt;    // [M] utterance index of each row
  const int32_t* pool_slotbase;   // [B]
  // generalised A addressing (2-D convolutions of the ResNet encoder on a zero-bordered NHWC grid,
  // model/resnet.py:25-79,217-261).  A[m, tap*ktap + kk] = X[a_off + m*a_pitch + tap*tap_stride + kk]
  // (element units).  a_pitch == 0 selects the default 1-D form above.  All of a_off, a_pitch,
  // tap_stride, ktap are multiples of 32 on the bf16x3 path (whole SB blocks).
  int64_t a_pitch;
  int64_t a_off;
  int64_t tap_stride;
  int ntaps;              // K == ntaps * ktap
  int ktap;
  // Gathered grid form (bf16x3 one-tap kernel only): GEMM row m reads the A row that starts at grid position arow[m]
  // (units of a_pitch elements) instead of position m, so the rows can enumerate just the output bins of a layer --
  // no MFMA work on border positions (csrc/grid.hip, rowmap_grid_compact_kernel).  arow is padded to a multiple of
  // 128 rows with position 0.
  const int32_t* arow;
  // residual shortcut added before the activation (resnet.py:84-85,147-148): fp32 [rows, N]
  const float* R;
  int64_t ldr;
  // ---- fused attentive pooling (model/pooling.py:189-217), bf16x3 kernel with the attention epilogue (EPI = 1):
  // (a) last key layer: instead of storing the key, every wave stores the partial scores of its 32 channels,
  //       att_part[((n / 32) * att_heads + h) * att_ld + m] = sum_{n' in block} act(...)[m, n'] * att_q[h * Npad + n']
  //     (att_q = the query expanded per head over the padded key width, zero outside the head's slice; the scale of
  //     :193-194 and the ordered sum over the blocks are applied by launch_att_scores_reduce);
  const float* att_q = nullptr;
  float* att_part = nullptr;
  int64_t att_ld = 0;
  int att_heads = 0;
  // (b) value layer: instead of storing the value, per 64-frame tile and utterance segment the weighted moments
  //       pool_part[(slot * 2 + 0) * pool_odim + oc] = sum_t w[t, h] x[t, c]
  //       pool_part[(slot * 2 + 1) * pool_odim + oc] = sum_t w[t, h] (x[t, c] - s1 / s0)^2,   s0 = sum_t w[t, h]
  //     with pool_w = the softmax output [rows, pool_heads]; split value (:151-157): h = c / pool_dvh, oc = c; else
  //     every head pools every channel, oc = h * N + c.  launch_att_pool_finalize merges the slots (weighted Chan).
  const float* pool_w = nullptr;
  int pool_heads = 0;
  int pool_split = 0;
  int pool_dvh = 0;
  int pool_odim = 0;
};

// fp32 MFMA (v_mfma_f32_32x32x2_f32) path.  aligned: ldx == cin (or K == cin), ldx % 4 == 0,
// K % 4 == 0, X 16-byte aligned and followed by >= 160 rows of readable slack.
hipError_t launch_gemm_f32(const GemmArgs& a, bool aligned, hipStream_t s);

// number of K slices launch_gemm_f32 will use for this shape (1 = no split); the caller provides
// `partial` of ksplit * M * Npad floats when > 1.
int gemm_f32_ksplit(int M, int Kpad, int Npad);

// Tail balancing of the bf16x3 kernel (1-D layers): when the last round of 128x128 tiles over the chip's 768
// workgroup slots would be nearly empty, its M tiles are split along K into `*splits` slices each (deterministic:
// raw partials + an ordered reduce).  Returns the partial workspace in bytes (0 = no tail handling).
// (cb_quant: a slice must hold a multiple of this many channel blocks -- the two-unit kernel takes them in pairs (5 taps) or quads (7))
int64_t gemm_bf16x3_tail_plan(int M, int Kpad, int Npad, int w, int* tail_mt, int* splits, int cb_quant = 1);

// fp32 frames -> split-blocked im2col rows for a small-cin first layer:
//   out row m, k < w*cin: x[(m + k / cin) * ldx + k % cin]; zero padded to ldsb columns.
hipError_t launch_im2col_sb(const float* x, int64_t ldx, int cin, int w, int64_t rows, void* out_sb, int ldsb, int f16,
                            int* ovf, hipStream_t s);

// The one-tap form of the same (rows of ldsb >= cin channels, one per feature row) fused with the per-utterance lower-range guard of
// the fp16 formats: one pass over the features.  max_len = the longest utterance (frames); feat_stage_sb_ok: the shapes it takes.
bool feat_stage_sb_ok(int ldsb, int batch);
hipError_t launch_feat_stage_sb(const float* x, int64_t ldx, int cin, const int32_t* offsets_dev, int batch, int max_len,
                                void* out_sb, int ldsb, int f16, int* flags, hipStream_t s);

// bf16x3 / f16x3 split path (3x v_mfma_f32_16x16x32_{bf16,f16} per product tile).
hipError_t launch_gemm_bf16x3(const GemmArgs& a, hipStream_t s);
// the first layer as staged split-blocked rows of ONE 32-channel block, at most 5 taps, Npad % 128 == 0, plain 1-D rows and none of
// residual / fused pooling / attention epilogues: walking workgroups with resident weights (gemm_first.hip), the sums of
// launch_gemm_bf16x3 in the same order.  *taken = false (and nothing launched) for every other shape: the caller uses the tile kernel.
hipError_t launch_gemm_first(const GemmArgs& a, hipStream_t s, bool* taken);
// two-unit split of the multi-tap convolutions (XV_PREC_F16F6: f16 hi*hi + two block-scaled fp6 cross terms), gemm_f16f6.hip
hipError_t launch_gemm_f16f6(const GemmArgs& a, hipStream_t s);
// reduce of a K-split tail whose slices hold raw sums (a.partial / a.tail_mt / a.ksplit in {2, 4, 8}; rows from M tile nMain on):
// BN scale / shift + activation, then the split-blocked rows or (a.ysb_f6) the two-unit block format
hipError_t launch_f6v2_tail_reduce(const GemmArgs& a, int nMain, hipStream_t s);
// split-blocked f16 rows -> the activation block format of gemm_f16f6.hip (same 128 bytes per (row, 32 channels))
hipError_t launch_f6_from_sb(const void* sb, void* out, int64_t rows, int nblk, hipStream_t s);

// rowmap for a valid convolution of width w over packed utterances:
//   in_off[b] = off0[b] - b*ctx_in  (rows of utterance b in the layer's input)
//   row r of utterance b at local frame t maps to out_off[b] + t if t < len_b - (w-1), else -1.
hipError_t launch_build_rowmap(const int32_t* off0, int B, int ctx_in, int w, int32_t* rowmap, int M,
                               hipStream_t s);

// statistics pooling (model/pooling.py:27-52):  out[b] = [mean_t x, sqrt(max-floor(var_t x))]
//   rows of utterance b: [off0[b] - b*ctx, off0[b+1] - (b+1)*ctx)
hipError_t launch_stat_pool(const float* x, int64_t ldx, int C, const int32_t* off0, int B, int ctx,
                            float* out, int64_t ldo, hipStream_t s);

// row -> utterance map for the fused pooling epilogue (rows of utterance b: [off0[b]-b*ctx, off0[b+1]-(b+1)*ctx))
hipError_t launch_build_row2utt(const int32_t* off0, int B, int ctx, int32_t* row2utt, int M, hipStream_t s);
// finalize of the fused statistics pooling: merge the per-segment (sum, M2) pairs of each utterance
hipError_t launch_pool_finalize(const float* part, int C, const int32_t* off0, int B, int ctx,
                                const int32_t* slotbase, float* out, int64_t ldo, hipStream_t s);

// ---- ResNet grid helpers (csrc/grid.hip).  A "grid" value holds, per utterance b, (L_b + 2) time rows of S positions
// of C channels with a zero border (S = F + 1, or F + 2 when a consumer reads it at frequency stride 2); utterance b
// starts at position (off0[b] + 2b) * S.
// rowmap of a conv whose GEMM rows enumerate (b, t', j): t' in [0, L_b + 2), j in [0, rows_per_t):
//   output bin iff t' < L_b and j < Fout, at position (off0[b]+2b)*So + (t'+1)*So + j + 1; the other rows fall on border
//   positions: encoded "write zeros" (-pos - 2) when cover (rows_per_t == So), else -1 (the caller zeroes the value)
hipError_t launch_build_rowmap_grid(const int32_t* off0, int B, int rows_per_t, int Fout, int So, int cover, int32_t* rowmap,
                                    int64_t M, hipStream_t s);
// the same when the convolution also strides time by 2 (off_in / off_out: frame offsets at the input / output time level;
// ktime 3 = 3x3 'same', 1 = 1x1 shortcut); rows that produce no output frame are skipped (-1)
hipError_t launch_build_rowmap_grid_ts(const int32_t* off_in, const int32_t* off_out, int B, int rows_per_t, int Fout, int So,
                                       int ktime, int32_t* rowmap, int64_t M, hipStream_t s);
// rowmap of conv5 (1 x F valid): rows enumerate padded time rows; valid iff 1 <= t' <= L_b -> frame off0[b]+t'-1
// compact enumeration of a grid convolution (rows = output bins only): arow[m] = window position, rowmap[m] = output position
hipError_t launch_build_rowmap_grid_compact(const int32_t* off_in, const int32_t* off_out, int B, int Sin, int So, int Fout,
                                            int sw, int st, int ktime, int32_t* arow, int32_t* rowmap, int64_t M, int64_t Mpad,
                                            hipStream_t s);
// zero the border positions (and one pitch behind the last row) of a grid value; chunks = 16-byte chunks per position
hipError_t launch_grid_zero_border(const int32_t* off0, int B, int64_t frames, int F, int S, int chunks_y, int chunks_sb,
                                   float* y, void* ysb, hipStream_t s);
hipError_t launch_build_rowmap_rows(const int32_t* off0, int B, int32_t* rowmap, int64_t M, hipStream_t s);
hipError_t launch_build_rowmap_trows(const int32_t* off0, int B, int So, int32_t* rowmap, int64_t M, hipStream_t s);
// rowmap of conv0 (rows = grid positions, pitch S): interior -> same position, border -> zeros at the same position
hipError_t launch_build_rowmap_interior(const int32_t* off0, int B, int F, int S, int32_t* rowmap, int64_t M, hipStream_t s);
// conv0 im2col: out SB row p (grid position of the OUTPUT), k = kh*3+kw < 9: x[t+kh-1][f+kw-1] or 0
hipError_t launch_im2col2d_sb(const float* x, int64_t ldx, const int32_t* off0, int B, int F, int S, int64_t P, void* out_sb,
                              int f16, int* ovf, hipStream_t s);
hipError_t launch_im2col2d_f32(const float* x, int64_t ldx, const int32_t* off0, int B, int F, int S, int64_t P, float* out,
                               hipStream_t s);
// 3x3 stride-1 'same' max-pool of a grid value [P, C] (fp32 in; fp32 and / or SB out, either may be null); borders -> 0
// conv0 of the ResNet (3x3 'same' on the 1-channel feature map, model/resnet.py:217-228) computed directly: fp32 FMAs, BN scale /
// shift + activation, fp32 and / or split-blocked grid output (pitch S, border positions zero).  wdir = [9][C] kernel, scale[C], shift[C].
hipError_t launch_conv0_direct(const float* x, int64_t ldx, const int32_t* off0, int B, int F, int S, int C, int64_t P,
                               const float* wdir, int act, const float* alpha, float* y, void* ysb, int ldsb, int f16, int* ovf,
                               float sb_mul, hipStream_t s);
hipError_t launch_grid_maxpool3x3(const float* x, const int32_t* off0, int B, int F, int S, int C, int64_t P, float* y,
                                  void* ysb, int ldsb, int f16, int* ovf, float sb_mul, hipStream_t s);
// grid [P, C] -> dense [sum L_b * F, C] (drops the zero border; test / endpoint output only)
hipError_t launch_grid_unpad_n(const float* grid, const int32_t* off0, int B, int F, int S, int C, int64_t frames, float* out,
                               hipStream_t s);

// sliding-window CMN + voiced-frame selection (csrc/frontend.hip); prefix: double [(frames + B) * dim] scratch
hipError_t launch_cmn_select(const float* x, int64_t ld, int dim, const int32_t* off, int B, double* prefix,
                             const int32_t* src, int64_t out_rows, int window, int center, int min_window, float* out,
                             hipStream_t s);

// MFCC + energy VAD (csrc/mfcc.hip; the opaque xv_mfcc of include/xvec_hip.h holds the tables).  mfcc_create validates the
// options (reason in *err) before any HIP call.
int mfcc_create(const xv_mfcc_opts* opts, int device, xv_mfcc** out, std::string* err);
void mfcc_destroy(xv_mfcc* m);
int mfcc_num_frames(const xv_mfcc* m, int64_t num_samples, int64_t* out);
int mfcc_device(const xv_mfcc* m);
int mfcc_num_ceps(const xv_mfcc* m);
hipError_t launch_mfcc(xv_mfcc* m, const int16_t* wave, const int64_t* sample_off, const int32_t* frame_off, int B, float* out,
                       int64_t ld, hipStream_t s);
hipError_t launch_vad_energy(const float* feats, int64_t ld, const int32_t* frame_off, int B, float threshold, float mean_scale,
                             int context, float proportion, float* vad, hipStream_t s);
// fbank (csrc/mfcc.hip, next to the MFCC it shares its frame steps with); log_energy may be null
int fbank_create(const xv_fbank_opts* opts, int device, xv_fbank** out, std::string* err);
void fbank_destroy(xv_fbank* m);
int fbank_num_frames(const xv_fbank* m, int64_t num_samples, int64_t* out);
int fbank_device(const xv_fbank* m);
int fbank_num_feats(const xv_fbank* m);
hipError_t launch_fbank(xv_fbank* m, const int16_t* wave, const int64_t* sample_off, const int32_t* frame_off, int B, float* out,
                        int64_t ld, float* log_energy, hipStream_t s);

// post-step (csrc/post.hip): ivector-normalize-length / ivector-mean of run_extract_embeddings.sh:80-103
hipError_t launch_length_norm(const float* x, int64_t ldx, int64_t rows, int dim, int scaleup, float* y, int64_t ldy,
                              hipStream_t s);
hipError_t launch_speaker_mean(const float* x, int64_t ldx, int dim, const int32_t* spk_off, const int32_t* utt,
                               int64_t num_spk, float* out, int64_t ldo, hipStream_t s);

// cosine scoring (csrc/score.hip): egs/voxceleb/v1/run.sh:362-365,404-408 and misc/utils.py:307-346
hipError_t compute_units(int* cus);     // of the current device: sizes the grids of the persistent tile kernels
// y = x - mean (mean may be null), then y / sqrt(sum y^2 + eps) when `normalize`; in place (y == x) is allowed
hipError_t launch_score_prepare_rows(const float* x, int64_t ldx, int64_t rows, int dim, const float* mean, int normalize,
                                     float eps, float* y, int64_t ldy, hipStream_t s);
// out[i, j] = sum_k (a[i, k] - a_sub[k]) * b[j, k] (+ b[j, d] when b_offset); a_sub may be null; 1 <= d <= 2048
hipError_t launch_score_matrix(const float* a, int64_t lda, int n, const float* b, int64_t ldb, int m, int d,
                               const float* a_sub, int b_offset, float* out, int64_t ldo, hipStream_t s);
// hs / hd [nbins] += counts of the scores a[i] . b[j] with la[i] == lb[j] / != ; `self`: only i < j
hipError_t launch_score_histogram(const float* a, int64_t lda, int n, const int32_t* la, const float* b, int64_t ldb, int m,
                                  const int32_t* lb, int d, int self, int nbins, unsigned long long* hs,
                                  unsigned long long* hd, hipStream_t s);
// out[k] = a[ia[k]] . b[ib[k]]; an index out of range writes NaN (the caller checks its indices on the host)
hipError_t launch_score_pairs(const float* a, int64_t lda, int n, const float* b, int64_t ldb, int m, int d, const int32_t* ia,
                              const int32_t* ib, int64_t npairs, float* out, hipStream_t s);

// PLDA scoring (csrc/score.hip; Kaldi's ivector-plda-scoring, egs/voxceleb/v1/run.sh:410-426): the row kernel behind the
// affine product (normalisation, packed operands, bias), and the PLDA forms of the three scoring launches, which add
// row_bias[i] + col_bias[j] (col_bias may be null) to the product of the packed rows; k = d or 2 d, 1 <= k <= 2048
hipError_t launch_plda_rows(const float* u, int64_t ldu, int64_t rows, int d, int norm, int side, int pack_second,
                            const double* tables, const double* logdet, const int32_t* table_index, int num_tables,
                            float* rows_out, int64_t ldr, float* packed, int64_t ldp, float* bias, hipStream_t s);
hipError_t launch_plda_matrix(const float* a, int64_t lda, int n, const float* row_bias, const float* b, int64_t ldb, int m,
                              const float* col_bias, int k, float* out, int64_t ldo, hipStream_t s);
hipError_t launch_plda_histogram(const float* a, int64_t lda, int n, const float* row_bias, const int32_t* la, const float* b,
                                 int64_t ldb, int m, const float* col_bias, const int32_t* lb, int k, double lo, double hi,
                                 int nbins, unsigned long long* hs, unsigned long long* hd, hipStream_t s);
hipError_t launch_plda_pairs(const float* a, int64_t lda, int n, const float* row_bias, const float* b, int64_t ldb, int m,
                             const float* col_bias, int k, const int32_t* ia, const int32_t* ib, int64_t npairs, float* out,
                             hipStream_t s);

// Cohort statistics for score normalisation (csrc/score.hip): per row i of a, mean and population std of the top_k largest
// scores a[i] . b[j] + row_bias[i] + col_bias[j] over the columns j with la[i] != lb[j] (top_k 0: all of them).  The scores go
// through a panel of whole tile rows in `ws` (at least cohort_stats_workspace_bytes), written by the matrix epilogues.
int64_t cohort_stats_workspace_bytes(int64_t n, int64_t m);
hipError_t launch_cohort_stats(const float* a, int64_t lda, int n, const float* row_bias, const int32_t* la, const float* b,
                               int64_t ldb, int m, const float* col_bias, const int32_t* lb, int k, int top_k, float* mean,
                               float* stdv, int32_t* count, void* ws, int64_t ws_bytes, hipStream_t s);

// Top-K search (csrc/score.hip): per row i of a, the top_k largest scores a[i] . b[j] + row_bias[i] + col_bias[j] over the
// columns j with la[i] != lb[j] and their columns, by score descending then column ascending, into scores / index [n, ldo]
// (padded with -inf / -1); count [n] (or null) gets the number of hits.  The panel and its workspace are the cohort call's.
int64_t score_topk_workspace_bytes(int64_t n, int64_t m);
hipError_t launch_score_topk(const float* a, int64_t lda, int n, const float* row_bias, const int32_t* la, const float* b,
                             int64_t ldb, int m, const float* col_bias, const int32_t* lb, int k, int top_k, float* scores,
                             int32_t* index, int64_t ldo, int32_t* count, void* ws, int64_t ws_bytes, hipStream_t s);

// Speaker clustering (csrc/cluster.hip): average-linkage AHC of every group's rows from its score matrix, one workgroup per group.
// rows / target are host arrays (target may be null: 1); ws holds ahc_workspace_bytes(num_groups) bytes and receives the group
// table, stream-ordered.  The caller has checked every argument; num_groups >= 1.
int64_t ahc_matrix_floats(int64_t n);
int64_t ahc_workspace_bytes(int64_t num_groups);
hipError_t launch_ahc(float* s, const int32_t* rows, const int32_t* target, int64_t num_groups, double threshold, int32_t* labels,
                      int32_t* num_clusters, int32_t* merge_a, int32_t* merge_b, double* merge_height, void* ws, hipStream_t stream);

// Per-recording PCA adaptation of a PLDA model (csrc/plda_adapt.hip): one workgroup per group, from the rows to the adapted
// affine.  offsets is a host array [num_groups + 1]; ws holds at least plda_adapt_workspace_bytes(num_groups, d) bytes (the
// offsets table and one slot; every further slot lets one more group run at a time).  The caller has checked every argument;
// num_groups >= 1.
int64_t plda_adapt_slot_bytes(int d);
int64_t plda_adapt_workspace_bytes(int64_t num_groups, int d);
hipError_t launch_plda_adapt(const float* x, int64_t ldx, const int64_t* offsets, int64_t num_groups, int d, const double* mean,
                             const double* within_factor, const double* psi, double target_energy, int32_t* dim, double* eigval,
                             double* pca, double* affine, double* psi_out, void* ws, int64_t ws_bytes, hipStream_t stream);

// VB-HMM resegmentation of x-vector sequences (csrc/vbx.hip): one projection launch over all rows, then one workgroup per
// group for all iterations.  offsets [num_groups + 1] and num_spk [num_groups] are host arrays; ws holds
// vbx_workspace_bytes(...) bytes and receives the group table, stream-ordered.  The caller has checked every argument;
// num_groups >= 1.
int64_t vbx_workspace_bytes(int64_t num_groups, const int64_t* offsets, const int32_t* num_spk, int r);
hipError_t launch_vbx(const float* x, int64_t ldx, const int64_t* offsets, const int32_t* num_spk, int64_t num_groups, int d,
                      const double* affine, const double* psi, int r, double* gamma, double* pi, double fa, double fb,
                      double loop_prob, int max_iters, double epsilon, int32_t* labels, double* elbo, int32_t* iters, void* ws,
                      hipStream_t stream);

// Metric-learning loss heads (csrc/metric_loss.hip): semi-hard triplet, angular triplet (all / hard), ge2e (softmax /
// contrastive), per group of rows.  offsets is a host array [num_groups + 1]; ws holds at least metric_loss_workspace_bytes
// bytes.  The caller has checked every argument (ascending offsets, 1 .. 4096 rows per group); num_groups >= 1.
int64_t metric_loss_slot_bytes(int max_rows, int d, int kind);
int64_t metric_loss_workspace_bytes(int64_t num_groups, const int64_t* offsets, int d, int kind);
hipError_t launch_metric_loss(const float* x, int64_t ldx, const int64_t* offsets, int64_t num_groups, int d, const int32_t* labels,
                              int kind, int pos_head, double margin, int squared, int normalize, double w, double b,
                              double* row_loss, int64_t* row_count, int32_t* row_top1, double* group_loss, int64_t* group_count,
                              void* ws, int64_t ws_bytes, hipStream_t stream);

// The triplet kinds with their gradient (csrc/metric_loss_grad.hip): the forward outputs of launch_metric_loss, bit for bit,
// and grad_x [total, ldg] = float32(grad_scale dL_g / dx).  The caller has checked every argument (kinds 0 .. 2, 1 .. 1024 rows
// per group); num_groups >= 1.
int64_t metric_loss_grad_workspace_bytes(int64_t num_groups, const int64_t* offsets, int d);
hipError_t launch_metric_loss_grad(const float* x, int64_t ldx, const int64_t* offsets, int64_t num_groups, int d,
                                   const int32_t* labels, int kind, int pos_head, double margin, int squared, int normalize,
                                   double grad_scale, double* row_loss, int64_t* row_count, double* group_loss, int64_t* group_count,
                                   float* grad_x, int64_t ldg, void* ws, int64_t ws_bytes, hipStream_t stream);

// classifier-head validation loss (csrc/loss.hip): model/loss.py:9-48,80-384 without the logit matrix
// kernel [E, ldk] -> class rows [C, ldr], columns normalised (tf.nn.l2_normalize) when `normalize`
hipError_t launch_loss_classes(const float* kernel, int64_t ldk, int E, int64_t C, int normalize, float* rows, int64_t ldr,
                               hipStream_t s);
int64_t loss_workspace_bytes(int64_t n, int64_t C);
// target[i] = the target logit after the margin (double arithmetic, rounded once); the first word of ws is zeroed and then
// set when a label lies outside [0, C) (that row gets NaN and is never followed)
hipError_t launch_loss_rows(const float* x, int64_t ldx, int64_t n, int E, const int32_t* labels, const float* rows, int64_t ldr,
                            int64_t C, const float* bias, int head, int m, double margin, double fa, float* target, void* ws,
                            hipStream_t s);
// tile kernel + merge: loss, lse, top1 [n] from x, the class rows and target; ws as sized by loss_workspace_bytes
hipError_t launch_loss_tiles(const float* x, int64_t ldx, int n, int E, const int32_t* labels, const float* rows, int64_t ldr, int C,
                             const float* bias, const float* target, float* loss, float* lse, int32_t* top1, void* ws,
                             hipStream_t s);

// loss and gradients of the classifier heads (csrc/loss_grad.hip).  ws as sized by loss_grad_workspace_bytes (least != 0: the
// smallest legal size, a panel of 32 rows).  _forward_rows normalises the raw rows into ws and evaluates the targets there; the
// first word of ws is the label flag of launch_loss_rows, to be read back before _rest is launched.
int64_t loss_grad_workspace_bytes(int64_t n, int64_t C, int E, int least);
hipError_t launch_loss_grad_forward_rows(const float* x, int64_t ldx, int64_t n, int E, const int32_t* labels, const float* rows,
                                         int64_t ldc, int64_t C, const float* bias, int head, int m, double margin, double fa,
                                         void* ws, hipStream_t s);
hipError_t launch_loss_grad_rest(const float* x, int64_t ldx, int n, int E, const int32_t* labels, const float* rows, int64_t ldc,
                                 int C, const float* bias, int head, int m, double margin, double fa, double grad_scale,
                                 float* loss, float* target, float* lse, int32_t* top1, float* grad_x, int64_t ldgx,
                                 float* grad_rows, float* grad_bias, void* ws, int64_t ws_bytes, hipStream_t s);

// one optimizer step on one float32 tensor (csrc/opt_step.hip); ws holds opt_workspace_bytes(count) bytes when clip_norm > 0
int64_t opt_workspace_bytes(int64_t count);
hipError_t launch_opt_step(int kind, int nesterov, float* w, const float* g, float* slot0, float* slot1, int64_t count, double lr,
                           double l2, double clip_norm, double momentum, int64_t step, void* ws, hipStream_t s);

// one segment-level layer, dense + inference-mode batch norm + activation, forward and backward (csrc/seg_grad.hip; the lines
// behind the product z, shared with csrc/tconv_grad.hip, and their bounds: csrc/layer_lines.h).  gamma, beta, mm, mv: all four or
// all null.  ws as sized by seg_workspace_bytes (least != 0: the smallest legal size, a panel of 64 rows).
int64_t seg_workspace_bytes(int64_t n, int K, int N, int least);
hipError_t launch_seg_forward(const float* x, int64_t ldx, int n, int K, const float* w, int64_t ldw, int N, const float* bias,
                              const float* gamma, const float* beta, const float* mm, const float* mv, int act, float* z, int64_t ldz,
                              float* y, int64_t ldy, hipStream_t s);
hipError_t launch_seg_backward(const float* gy, int64_t ldgy, const float* x, int64_t ldx, const float* z, int64_t ldz, int n, int K,
                               const float* w, int64_t ldw, int N, const float* gamma, const float* beta, const float* mm,
                               const float* mv, int act, float* gx, int64_t ldgx, float* gw, float* gbias, float* ggamma,
                               float* gbeta, void* ws, int64_t ws_bytes, hipStream_t s);

// one frame-level layer on packed utterances, W-tap temporal convolution + inference-mode batch norm + activation, forward and
// backward (csrc/tconv_grad.hip, csrc/layer_lines.h).  offsets [batch + 1] on the device; total_in and total_out are host bounds that size grids.
// ws as sized by tconv_workspace_bytes (the forward uses its first tconv_forward_workspace_bytes only).
int64_t tconv_workspace_bytes(int64_t batch, int64_t total_in, int64_t total_out, int W, int C, int N);
int64_t tconv_forward_workspace_bytes(int64_t batch, int64_t total_out);
hipError_t launch_tconv_forward(const float* x, int64_t ldx, int C, int W, const int32_t* offsets, int64_t batch, int64_t total_in,
                                int64_t total_out, const float* w, int64_t ldw, int N, const float* bias, const float* gamma,
                                const float* beta, const float* mm, const float* mv, int act, float* z, int64_t ldz, float* y,
                                int64_t ldy, void* ws, hipStream_t s);
hipError_t launch_tconv_backward(const float* gy, int64_t ldgy, const float* x, int64_t ldx, int C, int W, const int32_t* offsets,
                                 int64_t batch, int64_t total_in, int64_t total_out, const float* z, int64_t ldz, const float* w,
                                 int64_t ldw, int N, const float* gamma, const float* beta, const float* mm, const float* mv, int act,
                                 float* gx, int64_t ldgx, float* gw, float* gbias, float* ggamma, float* gbeta, void* ws,
                                 hipStream_t s);

// one grid convolution of the ResNet on packed utterances ((kh, kw) window, (st, sf) strides, 'same' padding; rows are utterance,
// frame, bin) + batch norm (inference mode) + activation, forward and backward, and the residual join y = act(p + q) with its
// gradient (csrc/gconv_grad.hip, csrc/layer_lines.h).  offsets [batch + 1] on the device counts frames; total_in and total_out are
// host bounds in frames.  bias and gbias may be null.  ws as sized by gconv_workspace_bytes (the forward uses its first
// gconv_forward_workspace_bytes only).  launch_add_act: gy null is the forward.
int64_t gconv_workspace_bytes(int64_t batch, int64_t total_in, int64_t total_out, int F_in, int kh, int kw, int st, int sf, int C,
                              int N);
int64_t gconv_forward_workspace_bytes(int64_t batch, int64_t total_out, int F_in, int sf);
hipError_t launch_gconv_forward(const float* x, int64_t ldx, int C, int F_in, int kh, int kw, int st, int sf, const int32_t* offsets,
                                int64_t batch, int64_t total_in, int64_t total_out, const float* w, int64_t ldw, int N,
                                const float* bias, const float* gamma, const float* beta, const float* mm, const float* mv, int act,
                                float* z, int64_t ldz, float* y, int64_t ldy, void* ws, hipStream_t s);
hipError_t launch_gconv_backward(const float* gy, int64_t ldgy, const float* x, int64_t ldx, int C, int F_in, int kh, int kw, int st,
                                 int sf, const int32_t* offsets, int64_t batch, int64_t total_in, int64_t total_out, const float* z,
                                 int64_t ldz, const float* w, int64_t ldw, int N, const float* gamma, const float* beta,
                                 const float* mm, const float* mv, int act, float* gx, int64_t ldgx, float* gw, float* gbias,
                                 float* ggamma, float* gbeta, void* ws, hipStream_t s);
hipError_t launch_add_act(const float* gy, int64_t ldgy, const float* p, int64_t ldp, const float* q, int64_t ldq, int64_t rows, int N,
                          int act, float* out, int64_t ldo, hipStream_t s);

// batch norm in training mode on the stored product z [n, N] of a trained layer: batch statistics, y, the moving averages in place
// (mm, mv: both or null), and the gradient through the statistics (csrc/bn_batch.hip, csrc/layer_lines.h)
int64_t bn_batch_workspace_bytes(int64_t n, int N);
hipError_t launch_bn_batch_forward(const float* z, int64_t ldz, int64_t n, int N, const float* gamma, const float* beta, int act,
                                   double momentum, int bessel, float* mm, float* mv, float* y, int64_t ldy, float* mean, float* var,
                                   void* ws, hipStream_t s);
hipError_t launch_bn_batch_backward(const float* gy, int64_t ldgy, const float* z, int64_t ldz, int64_t n, int N, const float* mean,
                                    const float* var, const float* gamma, const float* beta, int act, float* gz, int64_t ldgz,
                                    float* ggamma, float* gbeta, void* ws, hipStream_t s);

// statistics pooling of the caller's own packed rows and its gradient (csrc/pool_grad.hip); offsets [batch + 1] on the device,
// total_rows a host bound that sizes the backward's grid and clamps what an offset can reach
hipError_t launch_stat_pool_forward(const float* x, int64_t ldx, int C, const int32_t* offsets, int64_t batch, int64_t total_rows,
                                    float* pooled, int64_t ldp, float* var, int64_t ldv, hipStream_t s);
hipError_t launch_stat_pool_backward(const float* gp, int64_t ldgp, const float* x, int64_t ldx, int C, const int32_t* offsets,
                                     int64_t batch, int64_t total_rows, const float* pooled, int64_t ldp, const float* var,
                                     int64_t ldv, float* gx, int64_t ldgx, hipStream_t s);

// self-attentive pooling of the caller's own packed rows and its gradient (csrc/att_pool_grad.hip); dq and dv are the per-head
// widths, P = H dv; `panel` utterances of gquery partial sums fit the workspace (1 .. batch)
int64_t att_pool_workspace_bytes(int64_t batch, int64_t total_rows, int H, int dq, int P, int64_t panel);
hipError_t launch_att_pool_forward(const float* key, int64_t ldk, int dq, int split_k, const float* value, int64_t ldv, int dv,
                                   int split_v, const float* query, int64_t ldq, int H, float scale, const int32_t* offsets,
                                   int64_t batch, int64_t total_rows, float* w, int64_t ldw, float* pooled, int64_t ldp, float* var,
                                   int64_t ldvar, hipStream_t s);
hipError_t launch_att_pool_backward(const float* gp, int64_t ldgp, const float* key, int64_t ldk, int dq, int split_k,
                                    const float* value, int64_t ldv, int dv, int split_v, const float* query, int64_t ldq, int H,
                                    float scale, const int32_t* offsets, int64_t batch, int64_t total_rows, const float* w,
                                    int64_t ldw, const float* pooled, int64_t ldp, const float* var, int64_t ldvar, float* gkey,
                                    int64_t ldgk, float* gvalue, int64_t ldgv, float* gquery, int64_t ldgq, void* ws, int64_t ws_bytes,
                                    hipStream_t s);

// back-end training statistics (csrc/backend.hip): G = sum_r w_r (x_r - c)(x_r - c)^T in double (c, w may be null), both
// triangles of g [d, d]; ws holds gram_f64_workspace_bytes(n, d) bytes; rows fp32, or double in the _rows64 form
int64_t gram_f64_workspace_bytes(int64_t n, int d);
hipError_t launch_gram_f64(const float* x, int64_t ldx, int64_t n, int d, const double* c, const double* w, double* g,
                           double* ws, hipStream_t s);
hipError_t launch_gram_f64_rows64(const double* x, int64_t ldx, int64_t n, int d, const double* c, const double* w, double* g,
                                  double* ws, hipStream_t s);
// out[s] = mean of the rows index[off[s] .. off[s + 1]) of x [n, dim] in double, list order (- c when given); empty class: 0
hipError_t launch_class_mean_f64(const float* x, int64_t ldx, int64_t n, int dim, const int32_t* off, const int32_t* index,
                                 int64_t num_classes, const double* c, double* out, int64_t ldo, hipStream_t s);

// calibration statistics (csrc/calibrate.hip): F, g and the upper triangle of H of the prior-weighted logistic regression in
// double plus 19 int64 counters, see include/xvec_hip.h; theta [k + 1] and thresholds are host arrays, ws holds
// logreg_workspace_bytes(n, k) bytes.  launch_score_fuse: out[i] = float(llr_i)
int64_t logreg_workspace_bytes(int64_t n, int k);
hipError_t launch_logreg_stats(const float* scores, int64_t lds, int64_t n, int k, const uint8_t* targets, const double* theta,
                               double tau, double c_tar, double c_non, const double* thresholds, int num_thresholds, double* stats,
                               int64_t* counts, void* ws, hipStream_t s);
hipError_t launch_score_fuse(const float* scores, int64_t lds, int64_t n, int k, const double* theta, float* out, hipStream_t s);

// reverberation and additive noise (csrc/reverb.hip): the rule of include/xvec_hip.h on a packed batch.  utts / noises are host
// tables; reverb_validate checks them (XV_OK or an xv_status, message in *err) and nothing launches on a bad table; ws holds
// reverb_workspace_bytes bytes.  launch_reverb expects validated tables.
int64_t reverb_out_len(const xv_reverb_utt& u);
int reverb_validate(const xv_reverb_utt* utts, int64_t nu, const xv_reverb_noise* noises, int64_t nn, int64_t wave_samples,
                    int64_t rir_samples, int64_t noise_samples, int64_t out_samples, std::string* err);
int64_t reverb_workspace_bytes(const xv_reverb_utt* utts, int64_t nu, int64_t nn);
hipError_t launch_reverb(const int16_t* waves, const int16_t* rirs, const int16_t* sig, const xv_reverb_utt* utts, int64_t nu,
                         const xv_reverb_noise* noises, int64_t nn, int16_t* out16, float* out32, int32_t* status, int32_t* peak,
                         int32_t* clipped, void* ws, hipStream_t stream);

// attention scores (model/pooling.py:189-194): score[r, h] = scale * sum_d key[r, h*dk_h + d] * q[h, d]
// (split_key) or sum_d key[r, d] * q[h, d] (no split; dk_h == dk).
hipError_t launch_att_scores(const float* key, int64_t ldk, int64_t rows, const float* query, int H,
                             int dk_h, int split_key, float scale, float* scores, hipStream_t s);
// softmax over time per (utterance, head), in place on scores [rows, H]; also writes the
// [B, H, Lmax]-free packed layout weights_out[h * rows + r] when weights_out != nullptr.
hipError_t launch_att_softmax(float* scores, int H, const int32_t* off0, int B, int ctx, hipStream_t s);
// fused attention (csrc/xv_epilogue_n32.h, attention epilogue of the bf16x3 GEMM):
// scores[r, h] = scale * sum_blk part[(blk * H + h) * ld + r], blocks in ascending order (deterministic)
hipError_t launch_att_scores_reduce(const float* part, int64_t ld, int nblk, int H, int64_t rows, float scale,
                                    float* scores, hipStream_t s);
// per-slot weight sums for the weighted Chan merge: s0[slot * H + h] = sum of weights[r, h] over the rows of utterance b
// inside 64-row tile t, slot = slotbase[b] + t (rows in ascending order)
hipError_t launch_att_slot_sums(const float* weights, int H, const int32_t* off0, int B, int ctx, const int32_t* slotbase,
                                float* s0, hipStream_t s);
// out[b] = [sum_s s1 ..., sqrt(max-floor(sum_s m2_s + s0_s (s1_s / s0_s - mean)^2)) ...] over the slots of utterance b
hipError_t launch_att_pool_finalize(const float* part, const float* s0, int odim, int H, int dvh, int split,
                                    const int32_t* off0, int B, int ctx, const int32_t* slotbase, float* out, int64_t ldo,
                                    hipStream_t s);

// weighted mean / std (model/pooling.py:201-218).  value [rows, dv]; out[b] = [mean(h,d)..., std(h,d)...]
hipError_t launch_att_pool(const float* value, int64_t ldv, int dv, const float* weights, int H,
                           int split_value, const int32_t* off0, int B, int ctx, float* out, int64_t ldo,
                           hipStream_t s);

// y = act(x * scale[c] + shift[c]) on [rows, C] (att_post_bn / att_post_relu, stage replays)
hipError_t launch_affine_act(const float* x, int64_t ldx, int64_t rows, int C, const float* scale,
                             const float* shift, const float* alpha, int act, float* y, int64_t ldy,
                             hipStream_t s);

// l2_scaling (model/common.py:45-58): y = x * s * rsqrt(max(sum x^2, 1e-12)) per row
hipError_t launch_l2_scale(const float* x, int64_t rows, int C, float factor, float* y, hipStream_t s);

// transposed copy [B,H,L]-style attention weights: out[b][h][t] from scores [rows,H] (uniform L only)
hipError_t launch_copy2d(const float* src, int64_t lds, float* dst, int64_t ldd, int64_t rows, int cols,
                         hipStream_t s);
// fp16 range flags (2 ints) -> device-accessible host memory, then cleared; one kernel
hipError_t launch_flags_snapshot(int* dev, int* host, hipStream_t s);
// per-utterance lower-range feature guard (fp16 split formats): flag word kUttSmallWord of `flags` gets the largest |feature| of an
// utterance whose features are not all zero but all below 2^-8
hipError_t launch_feat_utt_guard(const float* x, int64_t ldx, int cin, const int32_t* offsets_dev, int batch, int* flags,
                                 hipStream_t s);
hipError_t launch_att_weights_out(const float* scores, int H, const int32_t* off0, int B, int ctx,
                                  float* out, hipStream_t s);

}  // namespace xv
