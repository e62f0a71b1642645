// LDS-staged epilogues of the 128-frame x 32-channel wave tile of the split-precision product kernels (the usual one with the
// fused statistics pooling, and the attention forms); the two block-format forms are in xv_f6.h.
#pragma once
#include "xv_epilogue.h"

namespace xv {

// 16-byte chunk `chunk` of staged frame `row` in a wave's scratch (128-byte rows, chunks swizzled by swz8(row))
__device__ __forceinline__ char* n32_slot(char* scratch, int row, int chunk) { return scratch + row * 128 + ((chunk ^ swz8(row)) << 4); }
// sum over the eight frame groups of a pass (lanes l, l ^ 8, l ^ 16, l ^ 32 hold the same channels)
__device__ __forceinline__ f32x4 n32_groups_sum(f32x4 v) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    v[i] += __shfl_xor(v[i], 8, 64);
    v[i] += __shfl_xor(v[i], 16, 64);
    v[i] += __shfl_xor(v[i], 32, 64);
  }
  return v;
}

// LDS-staged epilogue of a 128-frame x 32-channel wave tile acc[ft][ct] (8 x 2 accumulator tiles of 16 frames x 16
// channels, v_mfma_f32_16x16x32: lane & 15 -> frame, registers -> channels 4 * (lane >> 4) .. + 3; the "one wave per
// 32-channel block" layout of the split kernels).  A row of the wave tile is exactly one SB block
// (128 bytes) or 32 floats, so the scratch rows are 128 bytes (8 chunks, XOR-swizzled by swz8(frame), below) and the
// read-back hands 8 lanes one whole 128-byte line.  64 frames per pass (8 KB of scratch per wave): the partial slots of the
// fused statistics pooling are per 64-frame tile.
template <int ACT, bool F16>
__device__ __forceinline__ void store_wave_tile_n32_impl(const GemmArgs& p, const f32x4 (&acc)[8][2], int mbase, int nbase,
                                                         int lane, int wave, char* lds) {
  constexpr int ROWS = 64, NPASS = 2, FPP = 4;          // frames per pass, passes, 16-frame accumulator tiles per pass
  const int c16 = lane & 15, g4 = lane >> 4;
  char* scratch = lds + wave * (ROWS * 128);
  const int rrow = lane >> 3, rchunk = lane & 7;        // read-back map: 8 frames x 8 chunks per pass
  const f32x4 z = {0.f, 0.f, 0.f, 0.f};
  uint32_t bad = 0;                                     // F16 range guard: exponent-overflow bits of the converted hi halves

  // GemmArgs::sb_mul (the power of two the split-blocked copy is kept at): when that copy is the only output it is folded into
  // scale / shift here (every activation but tanh is positively homogeneous, and tanh layers have sb_mul == 1); otherwise the
  // values are multiplied right before their split (uniform branch)
  const bool fold = p.Ysb && !p.Y && !p.R && !p.pool_part && !p.raw;
  const float sbm = fold ? 1.f : p.sb_mul;
  f32x4 sc[2], sh[2];                                   // this lane's channels 16 ct + 4 g4 .. +3, ct = 0, 1
#pragma unroll
  for (int ct = 0; ct < 2; ++ct) {
    const int n4 = nbase + 16 * ct + 4 * g4;
    if (p.raw) {
      sc[ct] = f32x4{1.f, 1.f, 1.f, 1.f};
      sh[ct] = z;
    } else {
      const bool ok = n4 < p.N;
      sc[ct] = ok ? *reinterpret_cast<const f32x4*>(p.scale + n4) : z;
      sh[ct] = ok ? *reinterpret_cast<const f32x4*>(p.shift + n4) : z;
      if (fold) { sc[ct] *= p.sb_mul; sh[ct] *= p.sb_mul; }
    }
  }
  // Row map entries of every row this lane will store (8 per pass), loaded BEFORE the first store: vmcnt counts loads and
  // stores together and in order, so a row-map load issued behind the stores of the previous pass could only be consumed
  // once those stores are acknowledged (the convolutions' epilogue spent most of its time there).
  int rmap[NPASS][ROWS / 8];
#pragma unroll
  for (int ps = 0; ps < NPASS; ++ps)
#pragma unroll
    for (int it = 0; it < ROWS / 8; ++it) {
      const int m = mbase + ps * ROWS + it * 8 + rrow;
      rmap[ps][it] = rowmap_entry(p, m);
    }
  auto out_row_pre = [&](int ps, int it, bool& zero) -> int {      // out_row() on the preloaded entry
    return rowmap_decode(rmap[ps][it], zero);
  };
  XV_EPI_DRAIN();                                        // (trace builds: make the parameter-load latency visible)
  XV_EPI_STAMP(p, 4);
  auto value4 = [&](const f32x4& t, int ct, bool pre_act) -> f32x4 {
    f32x4 al = z;                                        // PReLU slopes: loaded at the point of use (registers are scarce)
    if (ACT < 0 && !pre_act && p.alpha && !p.raw && nbase + 16 * ct + 4 * g4 < p.N)
      al = *reinterpret_cast<const f32x4*>(p.alpha + nbase + 16 * ct + 4 * g4);
    f32x4 v;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float y = fmaf(t[i], sc[ct][i], sh[ct][i]);
      v[i] = pre_act ? y : apply_act(y, ACT < 0 ? p.act : ACT, al[i]);
    }
    return v;
  };
  auto stage_f32 = [&](int ps, bool pre_act) {          // fp32 chunk of channels 16 ct + 4 g4: index 4 ct + g4
#pragma unroll
    for (int fl = 0; fl < FPP; ++fl)
#pragma unroll
      for (int ct = 0; ct < 2; ++ct) {
        const int row = fl * 16 + c16;
        *reinterpret_cast<f32x4*>(n32_slot(scratch, row, 4 * ct + g4)) = value4(acc[ps * FPP + fl][ct], ct, pre_act);
      }
  };
  const int n = nbase + rchunk * 4;                      // read-back channels of this lane (fp32 forms)

  if (p.R) {
    const bool nok = n < p.N;
    const f32x4 al4 = (nok && p.alpha) ? *reinterpret_cast<const f32x4*>(p.alpha + n) : z;
#pragma unroll
    for (int ps = 0; ps < NPASS; ++ps) {
      stage_f32(ps, true);
      wave_lds_sync();
#pragma unroll 2
      for (int it = 0; it < ROWS / 8; ++it) {
        const int row = it * 8 + rrow;
        f32x4 v = *reinterpret_cast<const f32x4*>(n32_slot(scratch, row, rchunk));
        bool zero;
        const int orow = out_row_pre(ps, it, zero);
        if (orow < 0) continue;
        if (nok) {
          if (zero) {
            v = z;
          } else {
            v += *reinterpret_cast<const f32x4*>(p.R + (int64_t)orow * p.ldr + n);
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = apply_act(v[i], p.act, al4[i]);
          }
          if (p.Y) *reinterpret_cast<f32x4*>(p.Y + (int64_t)orow * p.ldy + n) = v;
        } else {
          v = z;
        }
        if (p.Ysb && n < p.ldsb) {
          uint32_t h01, l01, h23, l23;
          v *= p.sb_mul;
          split2t<F16>(v[0], v[1], h01, l01);
          split2t<F16>(v[2], v[3], h23, l23);
          if constexpr (F16) { ovf_bits(bad, h01); ovf_bits(bad, h23); }
          char* blk = reinterpret_cast<char*>(p.Ysb) + (int64_t)orow * p.ldsb * 4 + (n >> 5) * 128 + (n & 31) * 2;
          *reinterpret_cast<uint2*>(blk) = make_uint2(h01, h23);
          *reinterpret_cast<uint2*>(blk + 64) = make_uint2(l01, l23);
        }
      }
      wave_lds_sync();
    }
    if constexpr (F16) ovf_report_bits(p.ovf, bad);
    return;
  }
  if (p.Ysb) {
    const bool blk_ok = nbase < p.ldsb;                   // the SB block exists in the output row
#pragma unroll
    for (int ps = 0; ps < NPASS; ++ps) {
#pragma unroll
      for (int fl = 0; fl < FPP; ++fl)
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) {
          f32x4 v = value4(acc[ps * FPP + fl][ct], ct, false);   // padding channels: scale = shift = 0 -> 0
          if (sbm != 1.f) v *= sbm;
          uint32_t h01, l01, h23, l23;
          split2t<F16>(v[0], v[1], h01, l01);
          split2t<F16>(v[2], v[3], h23, l23);
          // channels 16 ct + 4 g4 .. + 3: bytes 32 ct + 8 g4 of the hi half (chunk 2 ct + g4 / 2), the same of the lo half
          const int row = fl * 16 + c16;
          if constexpr (F16) {                           // rows past M hold whatever the slack behind the input held
            if (mbase + ps * ROWS + row < p.M) { ovf_bits(bad, h01); ovf_bits(bad, h23); }
          }
          char* rp = scratch + row * 128 + 8 * (g4 & 1);
          *reinterpret_cast<uint2*>(rp + (((2 * ct + (g4 >> 1)) ^ swz8(row)) << 4)) = make_uint2(h01, h23);
          *reinterpret_cast<uint2*>(rp + (((4 + 2 * ct + (g4 >> 1)) ^ swz8(row)) << 4)) = make_uint2(l01, l23);
          if constexpr (F16) __builtin_amdgcn_sched_barrier(0);   // one tile at a time: the fp16 conversions of eight
                                                                  // interleaved tiles do not fit the register budget
        }
      wave_lds_sync();
      if (ps == 0) { XV_EPI_DRAIN(); XV_EPI_STAMP(p, 6); }
#pragma unroll 4
      for (int it = 0; it < ROWS / 8; ++it) {
        const int row = it * 8 + rrow;
        f32x4 v = *reinterpret_cast<const f32x4*>(n32_slot(scratch, row, rchunk));
        bool zero;
        const int orow = out_row_pre(ps, it, zero);
        if (zero) v = z;
        if (orow >= 0 && blk_ok)
          *reinterpret_cast<f32x4*>(reinterpret_cast<char*>(p.Ysb) + (int64_t)orow * p.ldsb * 4 + (nbase >> 5) * 128 +
                                    rchunk * 16) = v;
      }
      if (ps == 0) XV_EPI_STAMP(p, 7);
      wave_lds_sync();
    }
  }
  if constexpr (F16) ovf_report_bits(p.ovf, bad);
  XV_EPI_STAMP(p, 5);
  if (p.Y || p.pool_part) {
#pragma unroll
    for (int ps = 0; ps < NPASS; ++ps) {
      if (p.pool_part && !p.Y) {
        // Fused statistics pooling, the usual pass (all 64 frames of one utterance: 3.5 passes of 4.5 at 286 frames): straight from
        // the accumulators.  A lane holds 8 channels (2 tiles x 4) of the four frames c16 + 16 fl; the 16 lanes of a DPP row hold the
        // 16 frames of a tile row, so a channel's sum over the pass is four adds in-lane and a four-step butterfly across the row
        // (quad_perm, quad_perm, row_half_mirror, row_mirror: no LDS, no wait).  Same partials as the staged form below -- (sum, M2
        // about the pass mean) per (utterance, 64-frame tile) slot -- in another summation order.
        const int mb = mbase + ps * 64;
        const int my_utt = (mb + lane < p.M) ? p.pool_row2utt[mb + lane] : -1;
        const int u_first = __builtin_amdgcn_readlane(my_utt, 0), u_last = __builtin_amdgcn_readlane(my_utt, 63);
        if (u_first >= 0 && u_first == u_last) {
          auto row_sum = [&](float x) -> float {
            x += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0xB1, 0xF, 0xF, true));    // quad_perm [1,0,3,2]
            x += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x4E, 0xF, 0xF, true));    // quad_perm [2,3,0,1]
            x += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x141, 0xF, 0xF, true));   // row_half_mirror
            x += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x140, 0xF, 0xF, true));   // row_mirror
            return x;
          };
          const int64_t slot = (int64_t)p.pool_slotbase[u_first] + (mb >> 6);
#pragma unroll
          for (int ct = 0; ct < 2; ++ct) {
            f32x4 s1 = z;
#pragma unroll
            for (int fl = 0; fl < FPP; ++fl) s1 += value4(acc[ps * FPP + fl][ct], ct, false);
#pragma unroll
            for (int i = 0; i < 4; ++i) s1[i] = row_sum(s1[i]);
            const f32x4 mu = s1 * (1.0f / 64.0f);
            f32x4 m2 = z;
#pragma unroll
            for (int fl = 0; fl < FPP; ++fl) {
              const f32x4 d = value4(acc[ps * FPP + fl][ct], ct, false) - mu;
              m2 += d * d;
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) m2[i] = row_sum(m2[i]);
            const int nn = nbase + 16 * ct + 4 * g4;
            if (c16 == 0 && nn < p.N) store_moments(p.pool_part, slot, p.N, nn, s1, m2);
          }
          continue;
        }
      }
      stage_f32(ps, false);
      wave_lds_sync();
      if (ps == 0) XV_EPI_STAMP(p, 6);
      if (p.Y) {
#pragma unroll 4
        for (int it = 0; it < ROWS / 8; ++it) {
          const int row = it * 8 + rrow;
          f32x4 v = *reinterpret_cast<const f32x4*>(n32_slot(scratch, row, rchunk));
          bool zero;
          const int orow = out_row_pre(ps, it, zero);
          if (zero) v = z;
          if (orow >= 0 && n < p.N) *reinterpret_cast<f32x4*>(p.Y + (int64_t)orow * p.ldy + n) = v;
        }
      }
      if (p.pool_part) {
        // fused statistics pooling on the staged 64 frames x 32 channels (same (sum, M2 about the segment mean)
        // partials per (utterance, 64-frame tile) slot as the 64x64 form): lane = (frame group rrow = t mod 8,
        // 4 channels rchunk); the eight frame groups are combined with three xor-shuffles (n32_groups_sum).
        const int mb = mbase + ps * 64;
        const bool nok = n < p.N;
        const int my_utt = (mb + lane < p.M) ? p.pool_row2utt[mb + lane] : -1;
        const int tile64 = mb >> 6;
        auto row4 = [&](int t) -> f32x4 {
          return *reinterpret_cast<const f32x4*>(n32_slot(scratch, t, rchunk));
        };
        const int u_first = __builtin_amdgcn_readlane(my_utt, 0), u_last = __builtin_amdgcn_readlane(my_utt, 63);
        if (u_first >= 0 && u_first == u_last) {
          // the usual case: all 64 frames of the pass belong to one utterance (a 286-frame utterance has a boundary
          // in one pass out of 4.5).  Fixed trip counts: the eight rows of a lane are read back to back.
          f32x4 s1 = z;
#pragma unroll 4
          for (int k = 0; k < 8; ++k) s1 += row4(k * 8 + rrow);
          s1 = n32_groups_sum(s1);
          const f32x4 mu = s1 * (1.0f / 64.0f);
          f32x4 m2 = z;
#pragma unroll 4
          for (int k = 0; k < 8; ++k) {                 // second sweep of the LDS copy (registers are scarce here)
            const f32x4 d = row4(k * 8 + rrow) - mu;
            m2 += d * d;
          }
          m2 = n32_groups_sum(m2);
          if (nok && rrow == 0) store_moments(p.pool_part, (int64_t)p.pool_slotbase[u_first] + tile64, p.N, n, s1, m2);
        } else {
          // utterance boundaries (or the end of the matrix) inside the pass: one (sum, M2) pair per segment; the segment
          // ends come from one ballot per segment instead of a lane-by-lane scan
          int r = 0;
          while (r < 64) {
            const int b = __builtin_amdgcn_readlane(my_utt, r);
            const unsigned long long same = __ballot(my_utt == b) >> r;          // bit 0 = lane r (set)
            const int re = r + (~same ? __builtin_ctzll(~same) : 64 - r);
            if (b >= 0) {
              f32x4 s1 = z;
              for (int t0 = r & ~7; t0 < re; t0 += 8) {
                const int t = t0 + rrow;
                if (t >= r && t < re) s1 += row4(t);
              }
              s1 = n32_groups_sum(s1);
              const f32x4 mu = s1 / (float)(re - r);
              f32x4 m2 = z;
              for (int t0 = r & ~7; t0 < re; t0 += 8) {
                const int t = t0 + rrow;
                if (t >= r && t < re) {
                  const f32x4 d = row4(t) - mu;
                  m2 += d * d;
                }
              }
              m2 = n32_groups_sum(m2);
              if (nok && rrow == 0) store_moments(p.pool_part, (int64_t)p.pool_slotbase[b] + tile64, p.N, n, s1, m2);
            }
            r = re;
          }
        }
      }
      if (ps == 0) XV_EPI_STAMP(p, 7);
      wave_lds_sync();
    }
  }
}

// 1 / (weight sum of a slot segment) for the slot mean s1 / s0 of the weighted moments below.  Peaked attention leaves slots whose
// weights are all subnormal (softmax scores 88 .. 103 below the utterance's maximum): below 2^-128 the reciprocal overflows, the
// slot mean becomes inf (or 0 x inf) and the utterance's variance a NaN.  Such a slot carries less than 2^-126 of the weight: its
// moments are taken about zero instead (the merge in att_pool_finalize_kernel adds s0 (s1 / s0 - mean)^2 with a true division).
__device__ __forceinline__ float slot_inverse(float s0) { return s0 >= 1.17549435e-38f ? 1.0f / s0 : 0.f; }

// Attention epilogue of the 128-frame x 32-channel wave tile (kernel instantiations with EPI = 1; dense layers only:
// no rowmap).  Two forms, see GemmArgs:
//  * att_part: the tile is the last key layer's output and only its dot products with the query are wanted
//    (model/pooling.py:189-194).  A lane holds 8 channels of one frame per 16-frame tile row, so the partial score of
//    (frame, head) is 8 FMAs in-lane plus two exchanges across the four lane groups; the 16 frames of a tile
//    are stored as one 64-byte run.  The 1500-wide key never leaves the registers.
//  * pool_w: the tile is the value and only its weighted moments are wanted (:201-217): 64 frames are staged in the
//    wave-private LDS scratch as in the statistics form, then per utterance segment and head s1 = sum w x and
//    m2 = sum w (x - s1 / s0)^2 go to the segment's slot.
template <int ACT, int FORM>
__device__ __forceinline__ void store_wave_tile_n32_att_impl(const GemmArgs& p, const f32x4 (&acc)[8][2], int mbase, int nbase,
                                                             int lane, int wave, char* lds) {
  const int c16 = lane & 15, g4 = lane >> 4;
  const f32x4 z = {0.f, 0.f, 0.f, 0.f};
  f32x4 sc[2], sh[2];                                   // this lane's channels 16 ct + 4 g4 .. +3, ct = 0, 1
#pragma unroll
  for (int ct = 0; ct < 2; ++ct) {
    const int n4 = nbase + 16 * ct + 4 * g4;
    const bool ok = n4 < p.N;
    sc[ct] = ok ? *reinterpret_cast<const f32x4*>(p.scale + n4) : z;
    sh[ct] = ok ? *reinterpret_cast<const f32x4*>(p.shift + n4) : z;
  }
  auto value4 = [&](const f32x4& t, int ct) -> f32x4 {
    f32x4 al = z;                                        // PReLU slopes: loaded at the point of use (registers are scarce)
    if (ACT < 0 && p.alpha && nbase + 16 * ct + 4 * g4 < p.N) al = *reinterpret_cast<const f32x4*>(p.alpha + nbase + 16 * ct + 4 * g4);
    f32x4 v;
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = apply_act(fmaf(t[i], sc[ct][i], sh[ct][i]), ACT < 0 ? p.act : ACT, al[i]);
    return v;
  };
  if constexpr (FORM == 1) {
    const int blk = nbase >> 5;
#pragma unroll
    for (int ft = 0; ft < 8; ++ft) {
      f32x4 v[2];                                        // this lane's 8 channels of frame ft * 16 + c16, activated
#pragma unroll
      for (int ct = 0; ct < 2; ++ct) v[ct] = value4(acc[ft][ct], ct);   // padding channels: scale = shift = 0 and query 0
      const int m = mbase + ft * 16 + c16;
      for (int hd = 0; hd < p.att_heads; ++hd) {
        const float* qp = p.att_q + (int64_t)hd * p.Npad + nbase + 4 * g4;
        float s = 0.f;
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) {
          const f32x4 qv = *reinterpret_cast<const f32x4*>(qp + 16 * ct);
#pragma unroll
          for (int i = 0; i < 4; ++i) s = fmaf(v[ct][i], qv[i], s);
        }
        s += __shfl_xor(s, 16, 64);                      // the other 24 channels of this frame (lane groups g4)
        s += __shfl_xor(s, 32, 64);
        if (g4 == 0 && m < p.M) p.att_part[((int64_t)blk * p.att_heads + hd) * p.att_ld + m] = s;
      }
    }
    return;
  } else {
  // ---- weighted moments of the value
  char* scratch = lds + wave * (64 * 128);
  const int rrow = lane >> 3, rchunk = lane & 7;        // read-back map: 8 frames x 8 chunks per pass
  const int n = nbase + rchunk * 4;
  const bool nok = n < p.N;
  const int H = p.pool_heads;
  const int hd0 = p.pool_split ? min(nbase / p.pool_dvh, H - 1) : 0;     // split value: one head per 32-channel block
  const int hd1 = p.pool_split ? hd0 + 1 : H;
#pragma unroll
  for (int ps = 0; ps < 2; ++ps) {
#pragma unroll
    for (int fl = 0; fl < 4; ++fl)
#pragma unroll
      for (int ct = 0; ct < 2; ++ct) {
        const int row = fl * 16 + c16;
        *reinterpret_cast<f32x4*>(n32_slot(scratch, row, 4 * ct + g4)) = value4(acc[ps * 4 + fl][ct], ct);
      }
    wave_lds_sync();
    const int mb = mbase + ps * 64;
    const int my_utt = (mb + lane < p.M) ? p.pool_row2utt[mb + lane] : -1;
    const int tile64 = mb >> 6;
    auto row4 = [&](int t) -> f32x4 {
      return *reinterpret_cast<const f32x4*>(n32_slot(scratch, t, rchunk));
    };
    for (int hd = hd0; hd < hd1; ++hd) {
      const float wl = (mb + lane < p.M) ? p.pool_w[(int64_t)(mb + lane) * H + hd] : 0.f;   // lane = frame of this pass
      const int oc = p.pool_split ? n : hd * p.N + n;
      const int u_first = __builtin_amdgcn_readlane(my_utt, 0), u_last = __builtin_amdgcn_readlane(my_utt, 63);
      if (u_first >= 0 && u_first == u_last) {
        // all 64 frames of the pass belong to one utterance: fixed trip counts
        float s0 = wl;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s0 += __shfl_xor(s0, o, 64);
        float wt[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) wt[k] = __shfl(wl, k * 8 + rrow, 64);
        f32x4 s1 = z;
#pragma unroll 4
        for (int k = 0; k < 8; ++k) s1 += row4(k * 8 + rrow) * wt[k];
        s1 = n32_groups_sum(s1);
        const f32x4 mu = s1 * slot_inverse(s0);
        f32x4 m2 = z;
#pragma unroll 4
        for (int k = 0; k < 8; ++k) {                   // second sweep of the LDS copy (registers are scarce here)
          const f32x4 d = row4(k * 8 + rrow) - mu;
          m2 += d * d * wt[k];
        }
        m2 = n32_groups_sum(m2);
        if (nok && rrow == 0) store_moments(p.pool_part, (int64_t)p.pool_slotbase[u_first] + tile64, p.pool_odim, oc, s1, m2);
      } else {
        int r = 0;
        while (r < 64) {
          const int b = __builtin_amdgcn_readlane(my_utt, r);
          const unsigned long long same = __ballot(my_utt == b) >> r;          // bit 0 = lane r (set)
          const int re = r + (~same ? __builtin_ctzll(~same) : 64 - r);
          if (b >= 0) {
            float s0 = (lane >= r && lane < re) ? wl : 0.f;           // sum of the segment's weights
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) s0 += __shfl_xor(s0, o, 64);
            f32x4 s1 = z;
            for (int t0 = r & ~7; t0 < re; t0 += 8) {
              const int t = t0 + rrow;
              const float wt = __shfl(wl, t & 63, 64);
              if (t >= r && t < re) s1 += row4(t) * wt;
            }
            s1 = n32_groups_sum(s1);
            const f32x4 mu = s1 * slot_inverse(s0);
            f32x4 m2 = z;
            for (int t0 = r & ~7; t0 < re; t0 += 8) {
              const int t = t0 + rrow;
              const float wt = __shfl(wl, t & 63, 64);
              if (t >= r && t < re) {
                const f32x4 d = row4(t) - mu;
                m2 += d * d * wt;
              }
            }
            m2 = n32_groups_sum(m2);
            if (nok && rrow == 0) store_moments(p.pool_part, (int64_t)p.pool_slotbase[b] + tile64, p.pool_odim, oc, s1, m2);
          }
          r = re;
        }
      }
    }
    wave_lds_sync();
  }
  }
}

// FORM 1 = score partials (GemmArgs::att_part), 2 = weighted moments (GemmArgs::pool_w)
template <int FORM>
__device__ __forceinline__ void store_wave_tile_n32_att(const GemmArgs& p, const f32x4 (&acc)[8][2], int mbase, int nbase,
                                                        int lane, int wave, char* lds) {
  if (p.act == ACT_RELU)
    store_wave_tile_n32_att_impl<ACT_RELU, FORM>(p, acc, mbase, nbase, lane, wave, lds);
  else
    store_wave_tile_n32_att_impl<-1, FORM>(p, acc, mbase, nbase, lane, wave, lds);
}

template <bool F16>
__device__ __forceinline__ void store_wave_tile_n32(const GemmArgs& p, const f32x4 (&acc)[8][2], int mbase, int nbase,
                                                    int lane, int wave, char* lds) {
  if (wide_epilogue_ok(p)) {
    if (p.act == ACT_RELU)
      store_wave_tile_n32_impl<ACT_RELU, F16>(p, acc, mbase, nbase, lane, wave, lds);
    else if (p.act == ACT_NONE)
      store_wave_tile_n32_impl<ACT_NONE, F16>(p, acc, mbase, nbase, lane, wave, lds);
    else
      store_wave_tile_n32_impl<-1, F16>(p, acc, mbase, nbase, lane, wave, lds);
    return;
  }
#pragma unroll
  for (int ft = 0; ft < 8; ++ft)
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) store_tile16_scalar(p, acc[ft][ct], mbase + ft * 16, nbase + ct * 16, lane);
}

}  // namespace xv
