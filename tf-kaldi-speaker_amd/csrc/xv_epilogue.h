// GEMM epilogues (gfx950), the part every tile shape shares -- the row map, the scalar fallback stores, the wave-private LDS
// ordering point, the pooling slot store -- and the LDS-staged
// epilogue of the 64 x 64 wave tile of the fp32 kernel (32x32 accumulator layout).  The 128 x 32 wave tile of the
// split-precision product kernels (16x16 layout) is in xv_epilogue_n32.h.
#pragma once
#include "xv_common.h"

namespace xv {

// debug (tools/gemm_trace.py, -DXV_GEMM_TRACE builds only): phase stamps of the workgroup's first thread (0..3: the tile
// functions of gemm_bf16x3.hip, 4..7: the epilogues of xv_epilogue_n32.h)
#ifdef XV_GEMM_TRACE
#define XV_EPI_STAMP(p, i)                                                                                          \
  do {                                                                                                              \
    if ((p).trace && threadIdx.x == 0) (p).trace[(int64_t)blockIdx.x * 8 + (i)] = (long long)__builtin_amdgcn_s_memrealtime(); \
  } while (0)
#define XV_EPI_DRAIN() asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory")
#else
#define XV_EPI_STAMP(p, i) do {} while (0)
#define XV_EPI_DRAIN() do {} while (0)
#endif

// ---------------------------------------------------------------------------------------------
// Accumulator orientation used by every GEMM kernel here: the WEIGHT fragment is the MFMA A
// operand and the ACTIVATION fragment the B operand, so a 32x32 result tile is D[n][m]:
//   lane & 31            -> frame m (row of the output matrix)
//   (e&3) + 8*(e>>2) + 4*(lane>>5) -> channel n, i.e. registers 4q..4q+3 are FOUR CONSECUTIVE
//                                     channels 8q + 4*(lane>>5) .. +3 of one frame.
// A lane can therefore apply per-channel scale/shift with float4 loads, split to bf16 in packed
// pairs and emit 8/16-byte LDS writes with no cross-lane traffic.

// Row map.  Entry of GEMM row m: r >= 0 store at row r; -1 skip (also every m >= M); r <= -2 store ZEROS at row -r - 2 (a border
// position of a zero-bordered grid value that this GEMM row happens to cover: csrc/grid.hip -- this is what keeps the
// border zero without a memset of the whole output per layer).
__device__ __forceinline__ int rowmap_entry(const GemmArgs& p, int m) { return m < p.M ? (p.rowmap ? p.rowmap[m] : m) : -1; }
__device__ __forceinline__ int rowmap_decode(int r, bool& zero) {
  zero = r < -1;
  return zero ? -r - 2 : r;
}
// Output row of GEMM row m (-1: none), `zero`: store zeros there.
__device__ __forceinline__ int out_row(const GemmArgs& p, int m, bool& zero) {
  zero = false;
  if (m >= p.M) return -1;
  int r = p.rowmap ? p.rowmap[m] : m;
  if (r < -1) { zero = true; r = -r - 2; }
  return r;
}

// Scalar fallback (any N / alignment): one element at a time, fp32 and/or split-blocked.
__device__ __forceinline__ void store_tile_scalar(const GemmArgs& p, const f32x16& acc, int mbase, int nbase, int lane) {
  const int r32 = lane & 31, h = lane >> 5;
  const int m = mbase + r32;
  bool zero;
  const int orow = out_row(p, m, zero);
  if (orow < 0) return;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int n = nbase + (e & 3) + 8 * (e >> 2) + 4 * h;
    const bool nok = n < p.N;
    float v = 0.f;
    if (nok && !zero) {
      v = p.raw ? acc[e] : fmaf(acc[e], p.scale[n], p.shift[n]);
      if (p.R) v += p.R[(int64_t)orow * p.ldr + n];
      v = apply_act(v, p.raw ? ACT_NONE : p.act, p.alpha ? p.alpha[n] : 0.f);
    }
    if (p.Y && nok) p.Y[(int64_t)orow * p.ldy + n] = v;
    if (p.Ysb && n < p.ldsb) {
      uint32_t hi, lo;
      const float vs = v * p.sb_mul;
      split2(vs, 0.f, hi, lo, p.f16);
      if (p.f16 && !(fabsf(vs) <= kF16Max) && p.ovf) *p.ovf = 1;
      uint16_t* blk = reinterpret_cast<uint16_t*>(reinterpret_cast<char*>(p.Ysb) + (int64_t)orow * p.ldsb * 4 + (n >> 5) * 128);
      blk[n & 31] = (uint16_t)hi;
      blk[32 + (n & 31)] = (uint16_t)lo;
    }
  }
}

// The same for one 16x16 accumulator tile of the split kernels (lane & 15 -> frame, 4 * (lane >> 4) + i -> channel).
__device__ __forceinline__ void store_tile16_scalar(const GemmArgs& p, const f32x4& acc, int mbase, int nbase, int lane) {
  const int m = mbase + (lane & 15);
  bool zero;
  const int orow = out_row(p, m, zero);
  if (orow < 0) return;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int n = nbase + 4 * (lane >> 4) + e;
    const bool nok = n < p.N;
    float v = 0.f;
    if (nok && !zero) {
      v = p.raw ? acc[e] : fmaf(acc[e], p.scale[n], p.shift[n]);
      if (p.R) v += p.R[(int64_t)orow * p.ldr + n];
      v = apply_act(v, p.raw ? ACT_NONE : p.act, p.alpha ? p.alpha[n] : 0.f);
    }
    if (p.Y && nok) p.Y[(int64_t)orow * p.ldy + n] = v;
    if (p.Ysb && n < p.ldsb) {
      uint32_t hi, lo;
      const float vs = v * p.sb_mul;
      split2(vs, 0.f, hi, lo, p.f16);
      if (p.f16 && !(fabsf(vs) <= kF16Max) && p.ovf) *p.ovf = 1;
      uint16_t* blk = reinterpret_cast<uint16_t*>(reinterpret_cast<char*>(p.Ysb) + (int64_t)orow * p.ldsb * 4 + (n >> 5) * 128);
      blk[n & 31] = (uint16_t)hi;
      blk[32 + (n & 31)] = (uint16_t)lo;
    }
  }
}

// Ordering point between a wave's own LDS writes and its cross-lane read-back.  The scratch is private to the
// wave and DS instructions of one wave execute in order, so no workgroup barrier (and no s_barrier at all) is
// needed -- only that the compiler keeps the program order.
__device__ __forceinline__ void wave_lds_sync() {
  // No fence builtin here: on gfx950 vmcnt counts loads AND stores, and a release / acquire pair makes the compiler
  // drain it -- the wave would sit until the global stores of the previous pass are acknowledged (microseconds under
  // load) before it may restage the scratch.  Only compiler order (the asm memory clobber) and LDS order are needed.
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_wave_barrier();
}

// (sum, M2) of a segment into its slot of the pooling partials (rows of `ld` floats, columns col .. col + 3)
__device__ __forceinline__ void store_moments(float* part, int64_t slot, int ld, int col, const f32x4& s1, const f32x4& m2) {
  *reinterpret_cast<f32x4*>(part + (slot * 2) * ld + col) = s1;
  *reinterpret_cast<f32x4*>(part + (slot * 2 + 1) * ld + col) = m2;
}

// LDS-staged epilogue of a 64x64 wave tile acc[ni][mi] (2x2 MFMA tiles, orientation above).
// The wave writes its post-activation tile into a private LDS scratch shaped like the
// destination rows (256 bytes per frame: two SB blocks, or 64 floats; 16-byte chunks XOR-swizzled
// by frame & 15), then reads it back 16 bytes per lane and stores whole 256-byte row segments.
// All 64 frames are staged in one pass (16 KB of scratch per wave; the fused pooling needs the whole tile); the pass is still
// written as a one-trip loop: without the loop the compiler unrolls the sweeps inside it differently.
// Requirements (wide_epilogue_ok): N % 4 == 0, ldy % 4 == 0, 16-byte aligned Y.  `lds` is the workgroup's
// LDS base, 16 KB per wave, no longer read by the main loop (the caller's last K-loop barrier
// guarantees that); there is no workgroup barrier inside.
template <int ACT>
__device__ __forceinline__ void store_wave_tile_impl(const GemmArgs& p, const f32x16 (&acc)[2][2], int mbase, int nbase,
                                                     int lane, int wave, char* lds) {
  const int r32 = lane & 31, h = lane >> 5;
  char* scratch = lds + wave * (64 * 256);
  const int rrow = lane >> 4, rchunk = lane & 15;       // read-back map: 4 frames x 16 chunks
  auto slot = [&](int row, int chunk) -> char* { return scratch + row * 256 + ((chunk ^ (row & 15)) << 4); };

  auto value4 = [&](const f32x16& t, int q, const f32x4& sc, const f32x4& sh, const f32x4& al) -> f32x4 {
    f32x4 v;
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = apply_act(fmaf(t[4 * q + i], sc[i], sh[i]), ACT < 0 ? p.act : ACT, al[i]);
    return v;
  };
  auto params = [&](int n4, f32x4& sc, f32x4& sh, f32x4& al) {
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    if (p.raw) {                                    // split-K partial: accumulators unchanged
      sc = f32x4{1.f, 1.f, 1.f, 1.f};
      sh = z;
      al = z;
      return;
    }
    const bool ok = n4 < p.N;
    sc = ok ? *reinterpret_cast<const f32x4*>(p.scale + n4) : z;
    sh = ok ? *reinterpret_cast<const f32x4*>(p.shift + n4) : z;
    al = (ok && p.alpha) ? *reinterpret_cast<const f32x4*>(p.alpha + n4) : z;
  };
  // stage the fp32 values (post-activation unless `pre_act`): chunk ni*8 + 2q + h of frame row
  auto stage_f32 = [&](bool pre_act) {
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        f32x4 sc, sh, al;
        params(nbase + ni * 32 + 8 * q + 4 * h, sc, sh, al);
#pragma unroll
        for (int ml = 0; ml < 2; ++ml) {
          const int row = ml * 32 + r32;
          const f32x16& t = acc[ni][ml];
          f32x4 v;
          if (pre_act) {
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = fmaf(t[4 * q + i], sc[i], sh[i]);
          } else {
            v = value4(t, q, sc, sh, al);
          }
          *reinterpret_cast<f32x4*>(slot(row, ni * 8 + 2 * q + h)) = v;
        }
      }
  };

  if (p.R) {
    // residual form: stage the BN output in LDS, then add the fp32 shortcut row-wise (coalesced 16-byte loads), activate,
    // and store fp32 / SB.
    const int n = nbase + rchunk * 4;
    const bool nok = n < p.N;
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    const f32x4 al4 = (nok && p.alpha) ? *reinterpret_cast<const f32x4*>(p.alpha + n) : z;
#pragma unroll
    for (int ps = 0; ps < 1; ++ps) {
      stage_f32(true);
      wave_lds_sync();
#pragma unroll 4
      for (int it = 0; it < 16; ++it) {
        const int row = it * 4 + rrow;
        const int m = mbase + row;
        f32x4 v = *reinterpret_cast<const f32x4*>(slot(row, rchunk));
        bool zero;
        const int orow = out_row(p, m, zero);
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
          split2(v[0], v[1], h01, l01, p.f16);
          split2(v[2], v[3], h23, l23, p.f16);
          if (p.f16) ovf_report(p.ovf, fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fmaxf(fabsf(v[2]), fabsf(v[3]))));
          char* blk = reinterpret_cast<char*>(p.Ysb) + (int64_t)orow * p.ldsb * 4 + (n >> 5) * 128 + (n & 31) * 2;
          *reinterpret_cast<uint2*>(blk) = make_uint2(h01, h23);
          *reinterpret_cast<uint2*>(blk + 64) = make_uint2(l01, l23);
        }
      }
      wave_lds_sync();
    }
    return;
  }
  if (p.Ysb) {
    const bool blk_ok = nbase + (rchunk >> 3) * 32 < p.ldsb;     // SB block exists in the output row
#pragma unroll
    for (int ps = 0; ps < 1; ++ps) {
#pragma unroll
      for (int ni = 0; ni < 2; ++ni)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          f32x4 sc, sh, al;
          params(nbase + ni * 32 + 8 * q + 4 * h, sc, sh, al);     // padding channels: scale = shift = 0 -> 0
#pragma unroll
          for (int ml = 0; ml < 2; ++ml) {
            const f32x4 v = value4(acc[ni][ml], q, sc, sh, al) * p.sb_mul;
            uint32_t h01, l01, h23, l23;
            split2(v[0], v[1], h01, l01, p.f16);
            split2(v[2], v[3], h23, l23, p.f16);
            if (p.f16) ovf_report(p.ovf, fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fmaxf(fabsf(v[2]), fabsf(v[3]))));
            const int row = ml * 32 + r32;
            char* rp = scratch + row * 256 + 8 * h;                // (8-byte halves: slot() + 8 h)
            *reinterpret_cast<uint2*>(rp + (((ni * 8 + q) ^ (row & 15)) << 4)) = make_uint2(h01, h23);
            *reinterpret_cast<uint2*>(rp + (((ni * 8 + 4 + q) ^ (row & 15)) << 4)) = make_uint2(l01, l23);
          }
        }
      wave_lds_sync();
#pragma unroll 4
      for (int it = 0; it < 16; ++it) {
        const int row = it * 4 + rrow;
        const int m = mbase + row;
        f32x4 v = *reinterpret_cast<const f32x4*>(slot(row, rchunk));
        bool zero;
        const int orow = out_row(p, m, zero);
        if (zero) v = f32x4{0.f, 0.f, 0.f, 0.f};
        if (orow >= 0 && blk_ok)
          *reinterpret_cast<f32x4*>(reinterpret_cast<char*>(p.Ysb) + (int64_t)orow * p.ldsb * 4 + (nbase >> 5) * 128 +
                                    rchunk * 16) = v;
      }
      wave_lds_sync();
    }
  }
  if (p.Y || p.pool_part) {
    const int n = nbase + rchunk * 4;
#pragma unroll
    for (int ps = 0; ps < 1; ++ps) {
      stage_f32(false);
      wave_lds_sync();
      if (p.Y) {
#pragma unroll 4
        for (int it = 0; it < 16; ++it) {
          const int row = it * 4 + rrow;
          const int m = mbase + row;
          f32x4 v = *reinterpret_cast<const f32x4*>(slot(row, rchunk));
          bool zero;
          const int orow = out_row(p, m, zero);
          if (zero) v = f32x4{0.f, 0.f, 0.f, 0.f};
          if (orow >= 0 && n < p.N) *reinterpret_cast<f32x4*>(p.Y + (int64_t)orow * p.ldy + n) = v;
        }
      }
    }
  }
  if (p.pool_part) {
    // fused statistics pooling: lane = channel; for every utterance segment inside the 64-frame
    // tile store (sum x, sum (x - segment mean)^2) -- two passes over the LDS copy, so the merge in
    // pool_finalize_kernel (Chan et al.) is as accurate as the reference's two-pass variance.
    // Lane map: cq = lane & 15 -> columns 4cq..4cq+3 (one 16-byte LDS chunk), rg = lane >> 4 -> frames
    // t == rg (mod 4); the four frame groups are combined with two xor-shuffles.
    const int cq = lane & 15, rg = lane >> 4;
    const int n = nbase + 4 * cq;
    const bool nok = n < p.N;
    const int my_utt = (mbase + lane < p.M) ? p.pool_row2utt[mbase + lane] : -1;   // lane r: utterance of frame r
    const int tile64 = mbase >> 6;
    auto row4 = [&](int t) -> f32x4 { return *reinterpret_cast<const f32x4*>(slot(t, cq)); };
    auto groups_sum = [&](f32x4 v) -> f32x4 {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        v[i] += __shfl_xor(v[i], 16, 64);
        v[i] += __shfl_xor(v[i], 32, 64);
      }
      return v;
    };
    int r = 0;
    while (r < 64) {
      const int b = __builtin_amdgcn_readlane(my_utt, r);
      int re = r + 1;
      while (re < 64 && __builtin_amdgcn_readlane(my_utt, re) == b) ++re;
      if (b >= 0) {
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
        f32x4 s1 = z;
        for (int t0 = r & ~3; t0 < re; t0 += 4) {
          const int t = t0 + rg;
          if (t >= r && t < re) s1 += row4(t);
        }
        s1 = groups_sum(s1);
        const f32x4 mu = s1 / (float)(re - r);
        f32x4 m2 = z;
        for (int t0 = r & ~3; t0 < re; t0 += 4) {
          const int t = t0 + rg;
          if (t >= r && t < re) {
            const f32x4 d = row4(t) - mu;
            m2 += d * d;
          }
        }
        m2 = groups_sum(m2);
        if (nok && rg == 0) store_moments(p.pool_part, (int64_t)p.pool_slotbase[b] + tile64, p.N, n, s1, m2);
      }
      r = re;
    }
  }
}

// true when the vectorised LDS-staged epilogue applies to this launch
__device__ __forceinline__ bool wide_epilogue_ok(const GemmArgs& p) {
  return (p.N & 3) == 0 && (!p.Y || ((p.ldy & 3) == 0 && (reinterpret_cast<uintptr_t>(p.Y) & 15) == 0)) &&
         (!p.pool_part || p.rowmap == nullptr) &&
         (!p.R || ((p.ldr & 3) == 0 && (reinterpret_cast<uintptr_t>(p.R) & 15) == 0));
}

// Epilogue entry for a 64x64 wave tile: LDS-staged wide stores when the shape allows, scalar otherwise.
__device__ __forceinline__ void store_wave_tile(const GemmArgs& p, const f32x16 (&acc)[2][2], int mbase, int nbase,
                                                int lane, int wave, char* lds) {
  if (wide_epilogue_ok(p)) {
    if (p.act == ACT_RELU)
      store_wave_tile_impl<ACT_RELU>(p, acc, mbase, nbase, lane, wave, lds);
    else if (p.act == ACT_NONE)
      store_wave_tile_impl<ACT_NONE>(p, acc, mbase, nbase, lane, wave, lds);
    else
      store_wave_tile_impl<-1>(p, acc, mbase, nbase, lane, wave, lds);
    return;
  }
#pragma unroll
  for (int ni = 0; ni < 2; ++ni)
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) store_tile_scalar(p, acc[ni][mi], mbase + mi * 32, nbase + ni * 32, lane);
}

}  // namespace xv
