// Small device helpers shared by the GEMM epilogues and the kernels around them (pool.hip, grid.hip): vector types, the
// activation, the hi / lo split of the "split-blocked" (SB) activation format with its fp16 range guard, the MFMA wrappers,
// the scratch-row swizzle and the XCD remap.
//
// SB format: a row of C channels is stored as ceil(C/32) blocks of 128 bytes; block j holds
// channels 32j..32j+31 as [32 x bf16 hi | 32 x bf16 lo] with hi = rn_bf16(x), lo = rn_bf16(x - hi)
// (hi + lo carries 16 significant bits).  Same bytes per element as fp32; one (row, block) is
// one full 128-byte line, and 16-byte chunk q of a block is plane q>>2 (hi / lo), k chunk q&3 (= lane>>4) of the
// v_mfma_f32_16x16x32_bf16 A/B fragments.
#pragma once
#include "xv_kernels.h"

namespace xv {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef short bf16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ float apply_act(float v, int act, float alpha) {
  switch (act) {
    case ACT_RELU: return fmaxf(v, 0.0f);
    case ACT_LRELU: return fmaxf(v, kLreluAlpha * v);                       // tf.nn.leaky_relu
    case ACT_PRELU: return fmaxf(v, 0.0f) + alpha * (v - fabsf(v)) * 0.5f;  // model/common.py:40-42
    case ACT_TANH: return tanhf(v);
    default: return v;
  }
}

typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
typedef float f32x2_t __attribute__((ext_vector_type(2)));

typedef _Float16 f16x2_t __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// hi/lo split of two fp32 values, packed {a | b << 16}.
//  bf16 (F16 = false): v_cvt_pk_bf16_f32 (RNE, NaN-safe), shl/and, v_pk_add_f32, v_cvt_pk_bf16_f32 = 2.5 VALU per value;
//        hi + lo carries 16 significand bits over the full fp32 range.
//  fp16 (F16 = true):  hi = rn_f16(x), lo = rn_f16(x - hi): 22 significand bits for |x| in [2^-3, 65504]; below that the
//        low half goes subnormal (absolute error <= 2^-25), above it the value overflows to inf (the host checks).
template <bool F16>
__device__ __forceinline__ void split2t(float a, float b, uint32_t& hi, uint32_t& lo) {
  const f32x2_t v = {a, b};
  if constexpr (F16) {
    const f16x2_t hh = __builtin_convertvector(v, f16x2_t);
    hi = __builtin_bit_cast(uint32_t, hh);
    lo = __builtin_bit_cast(uint32_t, __builtin_convertvector(v - __builtin_convertvector(hh, f32x2_t), f16x2_t));
  } else {
    hi = __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2_t));
    const f32x2_t hf = {__uint_as_float(hi << 16), __uint_as_float(hi & 0xffff0000u)};
    lo = __builtin_bit_cast(uint32_t, __builtin_convertvector(v - hf, bf16x2_t));
  }
}
// fp16 range guard: callers fold every value they convert into `m` (one v_max3_f32 per pair) and report once per wave
constexpr float kF16Max = 65504.f;
__device__ __forceinline__ void ovf_track(float& m, float a, float b) { m = fmaxf(m, fmaxf(fabsf(a), fabsf(b))); }
__device__ __forceinline__ void ovf_report(int* flag, float m) {
  if (flag && !(m <= kF16Max)) *flag = 1;              // also true for NaN; every reporter writes the same value
}
// the same guard on the converted halves (hot epilogue: integer ops on registers that exist anyway, no extra live floats):
// a half is inf / NaN iff its exponent field is all ones, i.e. adding 1 to the field carries into the sign bit
__device__ __forceinline__ void ovf_bits(uint32_t& bad, uint32_t hi) { bad |= (hi & 0x7C007C00u) + 0x04000400u; }
__device__ __forceinline__ void ovf_report_bits(int* flag, uint32_t bad) {
  if (flag && (bad & 0x80008000u)) *flag = 1;
}
// run-time form for the kernels off the hot path (f16 is uniform over the launch)
__device__ __forceinline__ void split2(float a, float b, uint32_t& hi, uint32_t& lo, int f16) {
  if (f16) split2t<true>(a, b, hi, lo); else split2t<false>(a, b, hi, lo);
}

// one product tile of the split GEMM: v_mfma_f32_32x32x16_bf16 or _f16 (same rate, same fragment layout)
template <bool F16>
__device__ __forceinline__ f32x16 mfma_split(const bf16x8& a, const bf16x8& b, const f32x16& c) {
  if constexpr (F16)
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}

// The product kernels use the 16x16x32 shape: same FLOP per cycle as 32x32x16, but the chip holds a visibly higher clock
// on it under this load (MI355X_MICROARCH.md "DVFS give-back" item 7; measured in this kernel: profiles/README.md).
template <bool F16>
__device__ __forceinline__ f32x4 mfma_split16(const bf16x8& a, const bf16x8& b, const f32x4& c) {
  if constexpr (F16)
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

// XCD-aware bijective remap of a 1-D grid (ids congruent mod 8 share an XCD and its L2).
__device__ __forceinline__ int xcd_remap(int id, int n) {
  const int q = n >> 3, r = n & 7, x = id & 7, i = id >> 3;
  return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + i;
}

// Chunk swizzle of the 128-byte scratch rows of the 128 x 32 wave-tile epilogues: (row & 7) ^ ((row >> 3) & 1).  LDS stores see 32
// banks (one 128-byte row), so the eight consecutive rows of a ds_write_b128 lane group need eight different chunks: row & 7;
// loads see 64 banks (two rows) and serve a ds_read_b128 in groups of lanes {0-3, 12-15, 20-27} / {4-11, 16-19, 28-31}: with
// one row per lane (xv_f6.h) rows r and r + 24 / r + 12 of one parity would collide under row & 7 alone, bit 3 of the row
// separates them.  Measured (SQ_LDS_BANK_CONFLICT per 64-row pass): row & 7 alone 0 / 128 / 64 for the pooling / fp6 / split-
// blocked forms, (row >> 1) & 7 64 / 128 / 64; the split-blocked form's 64 are its ds_write_b64 (16 rows, one 8-byte half: 2-way
// by construction).  tests/analysis/lds_bank_model.py.
__device__ __forceinline__ int swz8(int row) { return (row & 7) ^ ((row >> 3) & 1); }

}  // namespace xv
