// C ABI of libxvec_hip.so, the executor: xv_forward walks the steps of a plan (api_plan.hip) and enqueues their kernels --
// launches only, no allocation, no host synchronisation (graph-capturable) -- and the optional per-step event profiler.
#include "xv_model.h"

using namespace xv;
using namespace xv::api;

namespace {

// One forward: what every step's launch needs besides the step itself.
struct Run {
  xv_handle* h;
  const xv_plan* p;
  const float* feats;
  int feat_ld;
  float* out;
  char* ws;               // aligned workspace base
  hipStream_t s;
  int f16;                // split format of the handle: fp16 hi/lo instead of bf16 hi/lo
  int B;
  const int32_t* off;     // frame offsets at time level 0
  // workspace offset -> pointer; a step's "none" (negative offset) is a null pointer
  char* raw(int64_t o) const { return o >= 0 ? ws + o : nullptr; }
  float* f32(int64_t o) const { return reinterpret_cast<float*>(raw(o)); }
  const float* in(int64_t o) const { return o == -2 ? feats : f32(o); }            // -2 = the network input
  float* dst(const PlanStep& st) const { return st.out_off >= 0 ? f32(st.out_off) : out; }
  int* ovf() const { return static_cast<int*>(h->ovf_flag.p); }
};

const char* step_name(const xv_handle* h, const PlanStep& st) {
  const Op& op = h->ops[st.op];
  switch (op.kind) {
    case OP_GEMM: {
      const Layer& L = h->layers[op.layer];
      if (!L.ep[ST_AFFINE].empty()) return L.ep[ST_AFFINE].c_str();
      const size_t a = L.kernel_name.find('/'), b = L.kernel_name.rfind('/');      // "resnet_18/conv1a_conv0/kernel"
      static thread_local std::string tmp;
      tmp = (a != std::string::npos && b > a) ? L.kernel_name.substr(a + 1, b - a - 1) : L.kernel_name;
      return tmp.c_str();
    }
    case OP_STAT_POOL: return "stat_pool";
    case OP_ATT_SCORES: return "att_scores";
    case OP_ATT_SOFTMAX: return "att_softmax";
    case OP_ATT_POOL: return "att_pool";
    case OP_AFFINE_ACT: return "att_post";
    case OP_L2_SCALE: return "l2_scale";
    case OP_GRID_MAXPOOL: return "conv0_max";
    default: return "op";
  }
}

// ------------------------------------------------------------------------------ OP_GEMM
// The GemmArgs fields that do not depend on which kernel runs the layer: operands, epilogue vectors, grid addressing,
// residual, the fused pooling / attention outputs and the split-blocked output.
GemmArgs gemm_args(const Run& r, const PlanStep& st, const Op& op, const Layer& L) {
  const xv_handle* h = r.h;
  const xv_model_desc& d = h->desc;
  GemmArgs a{};
  a.X = r.in(st.in0_off);
  a.ldx = op.in0 == 0 ? r.feat_ld : L.cin;
  a.cin = L.cin; a.M = st.M; a.K = L.K(); a.N = L.cout;
  a.Wt = static_cast<const float*>(L.wt.p); a.Kpad = L.Kpad; a.Npad = L.Npad;
  const bool bn_stage = st.stage >= ST_BN;
  a.scale = (bn_stage || !L.has_bn) ? L.d_scale() : L.d_ones();
  a.shift = (bn_stage || !L.has_bn) ? L.d_shift() : L.d_bias();
  a.act = (st.stage == ST_ACT) ? L.act : ACT_NONE;
  a.alpha = (a.act == ACT_PRELU) ? L.d_alpha() : nullptr;
  a.rowmap = st.rowmap >= 0 ? static_cast<const int32_t*>(r.p->d_rowmaps.p) + r.p->rowmap_off[st.rowmap] : nullptr;
  a.Y = r.dst(st); a.ldy = L.cout;
  a.f16 = r.f16;
  a.slab3 = h->opt_slab3;
  a.ovf = r.ovf();
  a.sb_mul = std::ldexp(1.f, L.out_exp);
  if (L.mode == 1 || L.mode == 2 || L.mode == 3) {      // A addressing on the input grid (csrc/grid.hip)
    const int64_t Sin = h->values[op.in0].grid_S;
    a.a_pitch = (L.mode == 3 ? Sin : L.sw) * (int64_t)L.cin;
    a.a_off = L.mode == 1 ? (L.sw == 1 ? 0 : L.cin) : (L.mode == 2 ? (Sin + 1) * L.cin : L.cin);
    if (st.compact()) {               // rows address their window through arow (units of one grid position)
      a.arow = static_cast<const int32_t*>(r.p->d_rowmaps.p) + r.p->rowmap_off[st.arow];
      a.a_pitch = L.cin;
      a.a_off = L.mode == 1 ? 0 : (Sin + 1) * L.cin;
    }
    a.ntaps = L.mode == 1 ? 3 : 1;
    a.ktap = L.mode == 1 ? 3 * L.cin : (L.mode == 2 ? L.cin : L.Fin * L.cin);
    a.tap_stride = Sin * L.cin;
    a.cin = a.K;                      // one "frame" per A row for the kernel's tap logic (w = 1)
  }
  if (op.in1 > 0) { a.R = r.in(st.in1_off); a.ldr = L.cout; }
  if (st.fuse_att == 1) {             // partial scores instead of the key (model/pooling.py:189-194)
    a.Y = nullptr;
    a.att_part = r.f32(st.out_off);
    a.att_ld = st.att_ld;
    a.att_heads = d.att_num_heads;
    a.att_q = static_cast<const float*>(h->query_eff.p);
  } else if (st.fuse_att == 2) {      // weighted moments instead of the value (:201-217)
    a.Y = nullptr;
    a.pool_part = r.f32(st.out_off);
    a.pool_row2utt = static_cast<const int32_t*>(r.p->d_row2utt.p);
    a.pool_slotbase = static_cast<const int32_t*>(r.p->d_slotbase.p);
    a.pool_w = r.f32(st.att_w_off);
    a.pool_heads = d.att_num_heads;
    a.pool_split = d.att_split_value;
    a.pool_dvh = d.att_split_value ? L.cout / d.att_num_heads : L.cout;
    a.pool_odim = h->pool_dim / 2;
  }
  if (st.fuse_pool) {                 // statistics pooling partials instead of activations
    a.Y = nullptr;
    a.pool_part = r.f32(st.out_off);
    a.pool_row2utt = static_cast<const int32_t*>(r.p->d_row2utt.p);
    a.pool_slotbase = static_cast<const int32_t*>(r.p->d_slotbase.p);
  }
  if (st.out_sb_off >= 0) {
    a.Ysb = r.raw(st.out_sb_off);
    a.ldsb = sb_ld(L.cout);
    if (st.out_off < 0 && !st.to_out) a.Y = nullptr;
  }
  return a;
}

// The border of a grid output must be zero.  Covered outputs: the layer's own zero-writing rows do it, except for the
// first utterance's top border row and first left border (S + 1 positions no GEMM row maps to); otherwise the whole value
// is zeroed first.  In the full enumeration (no compact rows, no time-row map) the 2 S + 2 slack positions behind the value
// are zeroed as well, see below: up to four memsets there (head or whole value, and slack; f32 and f16 copy each), one
// border kernel and no memset on the default path.
int gemm_clear_border(const Run& r, const PlanStep& st, const Layer& L, const Value& vo) {
  xv_handle* h = r.h;
  const size_t head = (size_t)vo.grid_S + 1;
  // (whole-value clear: one more time row than the value has -- with the shared border column the 3x3 window of
  // the last bin of the last utterance's bottom border row reads position (L + 2, 0), just behind the grid)
  const size_t rows0 = st.grid_cover && L.mode != 4 ? head : (st.grid_cover ? 0 : (size_t)st.rows_out + vo.grid_S);
  if (st.compact() || st.trows()) {     // border positions only
    XV_HIP(h, launch_grid_zero_border(r.p->dev_offsets(st.lvl_out), r.B, st.frames_out, vo.grid_F, vo.grid_S, L.cout / 4,
                                      sb_ld(L.cout) / 4, r.f32(st.out_off), r.raw(st.out_sb_off), r.s));
  } else {
    if (rows0 > 0) {
      if (st.out_off >= 0) XV_HIP(h, hipMemsetAsync(r.raw(st.out_off), 0, rows0 * L.cout * 4, r.s));
      if (st.out_sb_off >= 0) XV_HIP(h, hipMemsetAsync(r.raw(st.out_sb_off), 0, rows0 * sb_ld(L.cout) * 4, r.s));
    }
    // Full enumeration (xv_set_option "grid_compact" 0): a consumer's GEMM rows cover every position of this value, the bottom
    // border row of the last utterance included, and the 3x3 windows of those rows end two time rows and two positions behind
    // the value, in its slack (kSlackRows).  Their results are zeros or dropped, but the fp16 range guard of the epilogue sees
    // them before the row map does: over bytes that nobody wrote it raised the overflow flag of a forward whose every stored
    // value was in range.  No GEMM row of the producer maps there (its zero-writing rows end at position (L + 3, 0)), so the
    // 2 S + 2 positions behind the value are cleared here.
    const size_t tail = 2 * (size_t)vo.grid_S + 2;
    if (tail > (size_t)kSlackRows) return fail(h, XV_ERR_STATE, "grid pitch %d: the window overreach does not fit the slack", vo.grid_S);
    if (st.out_off >= 0) XV_HIP(h, hipMemsetAsync(r.f32(st.out_off) + (size_t)st.rows_out * L.cout, 0, tail * L.cout * 4, r.s));
    if (st.out_sb_off >= 0)
      XV_HIP(h, hipMemsetAsync(static_cast<char*>(r.raw(st.out_sb_off)) + (size_t)st.rows_out * sb_ld(L.cout) * 4, 0,
                               tail * sb_ld(L.cout) * 4, r.s));
  }
  return XV_OK;
}

// conv0: 3x3 on the 1-channel input = im2col (9 taps, padded to 32) + dense GEMM, or the direct kernel
int launch_conv0(const Run& r, const PlanStep& st, const Layer& L, const Value& vo, GemmArgs& a) {
  xv_handle* h = r.h;
  if (st.scratch_off < 0) return fail(h, XV_ERR_STATE, "conv0 has no scratch");
  a.cin = 32; a.K = 32;             // taps 9..31 are zero in both operands
  // split precisions, final stage, not the requested node: nine fp32 FMAs per output on the vector units, BN +
  // activation + split store fused (one pass over the 200 MB output instead of im2col rows + a one-step GEMM)
  const bool direct = L.use_split && !st.to_out && st.stage == L.final_stage() && L.cout % 8 == 0 &&
                      (st.out_sb_off < 0 || L.cout % 32 == 0) && L.cout <= 256 && L.wdir.p;
  if (direct) {
    XV_HIP(h, launch_conv0_direct(r.feats, r.feat_ld, r.off, r.B, L.Fout, vo.grid_S, L.cout, st.M, static_cast<const float*>(L.wdir.p),
                                  L.act, L.d_alpha(), r.f32(st.out_off), r.raw(st.out_sb_off), sb_ld(L.cout), r.f16, r.ovf(),
                                  a.sb_mul, r.s));
  } else if (L.use_split) {
    XV_HIP(h, launch_im2col2d_sb(r.feats, r.feat_ld, r.off, r.B, L.Fout, vo.grid_S, st.M, r.raw(st.scratch_off), r.f16, r.ovf(), r.s));
    a.Xsb = r.raw(st.scratch_off); a.ldsbx = 32; a.Wsb = L.wsb.p; a.Wfr = L.wfr.p;
    XV_HIP(h, launch_gemm_bf16x3(a, r.s));
  } else {
    XV_HIP(h, launch_im2col2d_f32(r.feats, r.feat_ld, r.off, r.B, L.Fout, vo.grid_S, st.M, r.f32(st.scratch_off), r.s));
    a.X = r.f32(st.scratch_off); a.ldx = 32;
    XV_HIP(h, launch_gemm_f32(a, true, r.s));
  }
  return XV_OK;
}

// 30-dim first layer on the split kernel: its input is the caller's fp32 feature matrix, staged per forward
int launch_first_layer(const Run& r, const PlanStep& st, const Layer& L, GemmArgs& a) {
  xv_handle* h = r.h;
  if (st.scratch_off < 0) return fail(h, XV_ERR_STATE, "im2col layer has no scratch");
  a.Xsb = r.raw(st.scratch_off);
  a.Wsb = L.wsb.p; a.Wfr = L.wfr.p;
  bool guarded = false;               // the staging pass has taken the per-utterance maxima itself
  if (L.cin_pad) {
    // the 30-dim feature rows become SB rows of one 32-channel block (9.8 MB for 256 x 300 frames instead of the
    // 48 MB of materialised 5-frame rows); the layer is then an ordinary 5-tap convolution over them
    const std::vector<int32_t>& ho = r.p->lvl_offsets[0];
    guarded = feat_stage_sb_ok(L.cin_pad, r.B) && (int)ho.size() == r.B + 1 && ho[r.B] == st.rows_in;
    if (guarded) {                    // staging and the per-utterance guard in one pass (csrc/pool.hip)
      int max_len = 0;
      for (int b = 0; b < r.B; ++b) max_len = std::max(max_len, ho[b + 1] - ho[b]);
      XV_HIP(h, launch_feat_stage_sb(r.feats, r.feat_ld, L.cin, r.off, r.B, max_len, r.raw(st.scratch_off), L.cin_pad, r.f16, r.ovf(), r.s));
    } else {
      XV_HIP(h, launch_im2col_sb(r.feats, r.feat_ld, L.cin, 1, st.rows_in, r.raw(st.scratch_off), L.cin_pad, r.f16, r.ovf(), r.s));
    }
    a.ldsbx = L.cin_pad;
    a.cin = L.cin_pad;
    a.K = L.w * L.cin_pad;
    a.ysb_f6 = st.out_f6 ? 1 : 0;
  } else {
    // materialise the w*cin-wide rows once (SB format, K padded to 32), then it is a dense layer on those rows
    XV_HIP(h, launch_im2col_sb(r.feats, r.feat_ld, L.cin, L.w, st.M, r.raw(st.scratch_off), L.Kpad, r.f16, r.ovf(), r.s));
    a.ldsbx = L.Kpad;
    a.cin = a.K;
  }
  if (r.f16 && !guarded) XV_HIP(h, launch_feat_utt_guard(r.feats, r.feat_ld, L.cin, r.off, r.B, r.ovf(), r.s));
  // one 32-channel block and at most 5 taps: workgroups that walk the M tiles with resident weights (csrc/gemm_first.hip; the
  // same sums, bit-identical output).  By default only where it measured faster, as the producer of the two-unit block format
  // (76 -> 62 us; with the split-blocked / fp32 epilogue the two kernels tie within the noise: profiles/first_layer.md);
  // xv_set_option "first_walk" 2 takes it for every shape it accepts, 0 never
  bool walked = false;
  if (L.cin_pad && (h->opt_first_walk > 1 || (h->opt_first_walk == 1 && a.ysb_f6))) XV_HIP(h, launch_gemm_first(a, r.s, &walked));
  if (!walked) XV_HIP(h, launch_gemm_bf16x3(a, r.s));
  return XV_OK;
}

// two-unit split: convert the split-blocked input (unless the producer wrote the block format), then the f16 + fp6 kernel
int launch_two_unit(const Run& r, const PlanStep& st, const Op& op, const Layer& L, GemmArgs& a) {
  xv_handle* h = r.h;
  if (st.in0_sb_off < 0 || st.scratch_off < 0) return fail(h, XV_ERR_STATE, "f16f6 layer %s has no input / scratch", L.kernel_name.c_str());
  if (st.in_f6) {                   // the producer wrote this layer's block format
    a.Xsb = r.raw(st.in0_sb_off);
  } else {
    XV_HIP(h, launch_f6_from_sb(r.raw(st.in0_sb_off), r.raw(st.scratch_off), st.rows_in, sb_ld(L.cin) / 32, r.s));
    a.Xsb = r.raw(st.scratch_off);
    // taps w .. 7 of a scaled MFMA have zero weights but still read rows m + w .. m + 7: behind the last input row that is
    // whatever the buffer held, and an E8M0 scale byte of 255 there is a NaN (NaN x 0 = NaN) -- eight rows are kept defined:
    // by the producer's epilogue when it wrote this format itself, by a memset behind the conversion pass otherwise
    XV_HIP(h, hipMemsetAsync(r.raw(st.scratch_off) + st.rows_in * (int64_t)sb_ld(L.cin) * 4, 0, (size_t)8 * sb_ld(L.cin) * 4, r.s));
  }
  a.ysb_f6 = st.out_f6 ? 1 : 0;
  a.ldsbx = sb_ld(L.cin);
  a.Wfr = L.wf6m.p;
  a.Wx6 = L.wf6x.p;
  if (st.trows()) {
    // 3 x 3 on the zero-bordered grid as three taps along time: a GEMM row = one padded time row of Sin positions, the window
    // of frequency bin j = the 3 cin contiguous channels from position j on; output row rowmap[m] + j of the value advanced by
    // one position (csrc/grid.hip, rowmap_trows_kernel)
    const int64_t Sin = h->values[op.in0].grid_S;
    a.a_pitch = 0; a.a_off = 0; a.arow = nullptr; a.ntaps = 0; a.ktap = 0; a.tap_stride = 0;
    a.ldsbx = Sin * L.cin;
    a.cin = 3 * L.cin;
    a.K = 9 * L.cin;
    a.nbin = L.Fout;
    a.bin_x_bytes = (int64_t)L.cin * 4;
    if (a.Ysb) a.Ysb = static_cast<char*>(a.Ysb) + (int64_t)a.ldsb * 4;
    if (a.Y) a.Y += a.ldy;
    if (a.R) a.R += a.ldr;
  }
  if (st.tail_mt > 0 && st.scratch2_off >= 0) {
    a.tail_mt = st.tail_mt;
    a.ksplit = st.ksplit;
    a.partial = r.f32(st.scratch2_off);
  }
  XV_HIP(h, launch_gemm_f16f6(a, r.s));
  return XV_OK;
}

// three-unit split (bf16x3 / f16x3 kernels) on a split-blocked input
int launch_split(const Run& r, const PlanStep& st, const Layer& L, GemmArgs& a) {
  xv_handle* h = r.h;
  if (st.in0_sb_off < 0) return fail(h, XV_ERR_STATE, "split layer %s has no split-blocked input", L.kernel_name.c_str());
  a.Xsb = r.raw(st.in0_sb_off);
  a.ldsbx = L.mode == 0 ? sb_ld(L.cin) : 0;
  a.Wsb = L.wsb.p; a.Wfr = L.wfr.p;
  a.ysb_f6 = st.out_f6 ? 1 : 0;
  if (st.tail_mt > 0 && st.scratch_off >= 0) {
    a.tail_mt = st.tail_mt;
    a.ksplit = st.ksplit;
    a.partial = r.f32(st.scratch_off);
  }
  XV_HIP(h, launch_gemm_bf16x3(a, r.s));
  return XV_OK;
}

int launch_fp32(const Run& r, const PlanStep& st, const Op& op, const Layer& L, GemmArgs& a) {
  xv_handle* h = r.h;
  if (st.ksplit > 1 && st.scratch_off >= 0) {
    a.ksplit = st.ksplit;
    a.partial = r.f32(st.scratch_off);
  }
  const bool aligned = op.in0 != 0 && (a.ldx % 4 == 0) && (a.K % 4 == 0);
  if (L.mode != 0 && !aligned)
    return fail(h, XV_ERR_UNSUPPORTED, "resnet convolution %s needs channel counts that are multiples of 4", L.kernel_name.c_str());
  XV_HIP(h, launch_gemm_f32(a, aligned, r.s));
  return XV_OK;
}

int run_gemm(const Run& r, const PlanStep& st, const Op& op) {
  xv_handle* h = r.h;
  const Layer& L = h->layers[op.layer];
  const Value& vo = h->values[op.out];
  GemmArgs a = gemm_args(r, st, op, L);
  int rc = vo.grid_F > 0 ? gemm_clear_border(r, st, L, vo) : XV_OK;
  if (rc != XV_OK) return rc;
  if (L.mode == 4) rc = launch_conv0(r, st, L, vo, a);
  else if (L.im2col) rc = launch_first_layer(r, st, L, a);
  else if (L.use_f6) rc = launch_two_unit(r, st, op, L, a);
  else if (L.use_split) rc = launch_split(r, st, L, a);
  else rc = launch_fp32(r, st, op, L, a);
  if (rc != XV_OK) return rc;
  // One tail for every form.  (The direct conv0 kernel and the staged first layer never reach it with unpad_to_out set: the
  // first is only taken when !st.to_out, the second writes a frame-level value, and unpad_to_out means a grid-valued target.)
  if (st.unpad_to_out)
    XV_HIP(h, launch_grid_unpad_n(r.f32(st.out_off), r.p->dev_offsets(st.lvl_out), r.B, vo.grid_F, vo.grid_S, vo.cols, st.frames_out,
                                  r.out, r.s));
  return XV_OK;
}

// ------------------------------------------------------------------------------ one step
int run_step(const Run& r, const PlanStep& st) {
  xv_handle* h = r.h;
  const xv_plan* p = r.p;
  const xv_model_desc& d = h->desc;
  const Op& op = h->ops[st.op];
  const int B = r.B;
  const int32_t* off = r.off;
  hipStream_t s = r.s;
  float* optr = r.dst(st);
  const int32_t* off_in = p->dev_offsets(st.lvl_in);      // frame offsets at the time level of the step's input / output
  const int32_t* off_out = p->dev_offsets(st.lvl_out);
  switch (op.kind) {
    case OP_GEMM:
      return run_gemm(r, st, op);
    case OP_STAT_POOL: {
      const Value& vi = h->values[op.in0];
      if (st.fuse_pool) {
        XV_HIP(h, launch_pool_finalize(r.in(st.in0_off), vi.cols, off_in, B, vi.ctx,
                                       static_cast<const int32_t*>(p->d_slotbase.p), optr, 2 * vi.cols, s));
        break;
      }
      XV_HIP(h, launch_stat_pool(r.in(st.in0_off), vi.cols, vi.cols, off_in, B, vi.ctx, optr, 2 * vi.cols, s));
      break;
    }
    case OP_ATT_SCORES: {
      const Value& vi = h->values[op.in0];
      const float scale = d.att_use_scale ? 1.0f / std::sqrt((float)h->att_dk_h) : 1.0f;   // model/pooling.py:193-194
      if (st.fuse_att) {
        XV_HIP(h, launch_att_scores_reduce(r.in(st.in0_off), st.att_ld, h->key_npad / 32, d.att_num_heads, st.rows_in,
                                           scale, r.f32(st.out_off), s));
        break;
      }
      XV_HIP(h, launch_att_scores(r.in(st.in0_off), vi.cols, st.rows_in, static_cast<const float*>(h->query.p),
                                  d.att_num_heads, h->att_dk_h, d.att_split_key, scale, r.f32(st.out_off), s));
      break;
    }
    case OP_ATT_SOFTMAX: {
      float* sc = r.f32(st.out_off);
      XV_HIP(h, launch_att_softmax(sc, d.att_num_heads, off, B, h->final_ctx, s));
      if (st.fuse_att)
        XV_HIP(h, launch_att_slot_sums(sc, d.att_num_heads, off, B, h->final_ctx, static_cast<const int32_t*>(p->d_slotbase.p),
                                       r.f32(st.att_s0_off), s));
      if (st.to_out) XV_HIP(h, launch_att_weights_out(sc, d.att_num_heads, off, B, h->final_ctx, r.out, s));
      break;
    }
    case OP_ATT_POOL: {
      const Value& vv = h->values[op.in0];
      if (st.fuse_att) {
        XV_HIP(h, launch_att_pool_finalize(r.in(st.in0_off), r.f32(st.att_s0_off),
                                           h->pool_dim / 2, d.att_num_heads, d.att_split_value ? vv.cols / d.att_num_heads : vv.cols,
                                           d.att_split_value, off, B, vv.ctx, static_cast<const int32_t*>(p->d_slotbase.p),
                                           optr, h->pool_dim, s));
        break;
      }
      XV_HIP(h, launch_att_pool(r.in(st.in0_off), vv.cols, vv.cols, r.in(st.in1_off), d.att_num_heads,
                                d.att_split_value, off, B, vv.ctx, optr, h->pool_dim, s));
      break;
    }
    case OP_AFFINE_ACT: {
      const int n = h->pool_dim;
      const float* vec = static_cast<const float*>(h->post_vec.p);
      const int a = st.stage >= 2 ? act_of(d) : ACT_NONE;
      XV_HIP(h, launch_affine_act(r.in(st.in0_off), n, B, n, vec, vec + n,
                                  (a == ACT_PRELU) ? vec + 2 * n : nullptr, a, optr, n, s));
      break;
    }
    case OP_GRID_MAXPOOL: {
      const Value& vo = h->values[op.out];
      float* y = r.f32(st.out_off);
      // 2 S + 2 positions more than the value has: the kernel writes zeros there (they lie below the last utterance's bottom
      // border, in the slack), which is what the windows of a fully enumerating consumer's last GEMM rows read (see
      // gemm_clear_border) -- written by the producer, no memset
      const int64_t tail = 2 * (int64_t)vo.grid_S + 2;
      if (tail > kSlackRows) return fail(h, XV_ERR_STATE, "grid pitch %d: the window overreach does not fit the slack", vo.grid_S);
      XV_HIP(h, launch_grid_maxpool3x3(r.in(st.in0_off), off, B, vo.grid_F, vo.grid_S, vo.cols, st.rows_out + tail, y,
                                       r.raw(st.out_sb_off), sb_ld(vo.cols), r.f16, r.ovf(), std::ldexp(1.f, vo.sb_exp), s));
      if (st.unpad_to_out)
        XV_HIP(h, launch_grid_unpad_n(y, off_out, B, vo.grid_F, vo.grid_S, vo.cols, st.frames_out, r.out, s));
      break;
    }
    case OP_L2_SCALE: {
      XV_HIP(h, launch_l2_scale(r.in(st.in0_off), B, h->values[op.out].cols, d.feature_scaling_factor, optr, s));
      break;
    }
    default:
      return fail(h, XV_ERR_STATE, "unknown op kind %d", op.kind);
  }
  return XV_OK;
}

int run_plan(xv_handle* h, const xv_plan* p, const float* feats, int feat_ld, float* out, int64_t out_cap,
             void* workspace, int64_t ws_bytes, hipStream_t s) {
  if (!h || !p) return fail(h, XV_ERR_INVALID, "xv_forward: null handle/plan");
  if (p->h != h) return fail(h, XV_ERR_INVALID, "xv_forward: plan belongs to another handle");
  if (!feats || !out) return fail(h, XV_ERR_INVALID, "xv_forward: null feature/output pointer");
  if (feat_ld < h->desc.feat_dim) return fail(h, XV_ERR_INVALID, "xv_forward: feat_ld %d < feature_dim %d", feat_ld, h->desc.feat_dim);
  if (out_cap < p->info.out_rows * p->info.out_cols)
    return fail(h, XV_ERR_WORKSPACE, "xv_forward: output capacity %lld < %lld", (long long)out_cap,
                (long long)(p->info.out_rows * p->info.out_cols));
  if (ws_bytes < p->info.workspace_bytes || (!workspace && p->info.workspace_bytes > 0))
    return fail(h, XV_ERR_WORKSPACE, "xv_forward: workspace %lld bytes < %lld", (long long)ws_bytes, (long long)p->info.workspace_bytes);
  DeviceGuard g(h->device);
  if (!g.ok) return fail(h, XV_ERR_HIP, "cannot select HIP device %d", h->device);
  Run r{};
  r.h = h; r.p = p; r.feats = feats; r.feat_ld = feat_ld; r.out = out; r.s = s;
  r.ws = reinterpret_cast<char*>(align_up((int64_t)reinterpret_cast<uintptr_t>(workspace), kAlign));
  r.f16 = h->desc.precision == XV_PREC_F16X3 || h->desc.precision == XV_PREC_F16F6;
  r.B = p->info.batch;
  r.off = static_cast<const int32_t*>(p->d_offsets.p);

  bool prof = false;
  size_t prof_base = 0;
  if (h->profiling) {                     // reserve this forward's events under the lock; record them outside it
    std::lock_guard<std::mutex> lk(h->prof_mu);
    if (h->profiling && h->prof_next + 2 * p->steps.size() <= h->prof_pool.size()) {
      prof = true;
      prof_base = h->prof_next;
      h->prof_next += 2 * p->steps.size();
      h->prof_forwards++;
    }
  }

  for (size_t si = 0; si < p->steps.size(); ++si) {
    hipEvent_t pe0 = nullptr, pe1 = nullptr;
    const bool prof_step = prof && (!h->opt_profile_dominant || (int)si == p->dominant_step);
    if (prof_step) {
      pe0 = h->prof_pool[prof_base + 2 * si];
      pe1 = h->prof_pool[prof_base + 2 * si + 1];
      XV_HIP(h, hipEventRecord(pe0, s));
    }
    const int rc = run_step(r, p->steps[si]);
    if (rc != XV_OK) return rc;
    if (prof_step) {
      XV_HIP(h, hipEventRecord(pe1, s));
      std::lock_guard<std::mutex> lk(h->prof_mu);
      h->prof_recs.push_back({pe0, pe1, p, (int)si});
    }
  }
  return XV_OK;
}

}  // namespace

extern "C" {

int xv_forward(xv_handle* h, const xv_plan* p, const float* feats_dev, int feat_ld, float* out_dev, int64_t out_capacity,
               void* workspace, int64_t workspace_bytes, void* stream) {
  return run_plan(h, p, feats_dev, feat_ld, out_dev, out_capacity, workspace, workspace_bytes,
                  static_cast<hipStream_t>(stream));
}

int xv_profile_begin(xv_handle* h, int max_events) {
  if (!h) return fail(nullptr, XV_ERR_INVALID, "xv_profile_begin: null handle");
  if (max_events < 2) return fail(h, XV_ERR_INVALID, "xv_profile_begin: max_events < 2");
  DeviceGuard g(h->device);
  std::lock_guard<std::mutex> lk(h->prof_mu);
  while ((int)h->prof_pool.size() < max_events) {
    hipEvent_t e;
    XV_HIP(h, hipEventCreate(&e));
    h->prof_pool.push_back(e);
  }
  h->prof_next = 0;
  h->prof_recs.clear();
  h->prof_forwards = 0;
  h->profiling = true;
  return XV_OK;
}

int xv_profile_end(xv_handle* h, xv_kernel_time* entries, int max_entries, int* n_forwards) {
  if (!h) return fail(nullptr, XV_ERR_INVALID, "xv_profile_end: null handle");
  if (!h->profiling) return fail(h, XV_ERR_STATE, "xv_profile_end without xv_profile_begin");
  if (!entries || max_entries < 1) return fail(h, XV_ERR_INVALID, "xv_profile_end: no entry buffer");
  DeviceGuard g(h->device);
  std::lock_guard<std::mutex> lk(h->prof_mu);
  h->profiling = false;
  int n = 0;
  std::vector<int> count;
  for (const auto& r : h->prof_recs) {
    XV_HIP(h, hipEventSynchronize(r.e1));
    float ms = 0.f;
    XV_HIP(h, hipEventElapsedTime(&ms, r.e0, r.e1));
    const PlanStep& st = r.plan->steps[r.step];
    const char* name = step_name(h, st);
    int i = 0;
    for (; i < n; ++i)
      if (strncmp(entries[i].name, name, sizeof(entries[i].name) - 1) == 0 && entries[i].flops == st.flops) break;
    if (i == n) {
      if (n >= max_entries) continue;
      memset(&entries[n], 0, sizeof(xv_kernel_time));
      snprintf(entries[n].name, sizeof(entries[n].name), "%s", name);
      entries[n].flops = st.flops;
      entries[n].bytes = st.bytes;
      count.push_back(0);
      ++n;
    }
    entries[i].ms += ms;
    count[i]++;
  }
  for (int i = 0; i < n; ++i) {
    entries[i].launches = count[i];
    if (count[i] > 0) entries[i].ms /= (float)count[i];
  }
  if (n_forwards) *n_forwards = h->prof_forwards;
  h->prof_recs.clear();
  return n;
}

}  // extern "C"
