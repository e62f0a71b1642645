// The pieces of the metric-learning heads that csrc/metric_loss.hip (the forward) and csrc/metric_loss_grad.hip (the forward
// with its gradient) share, so that both give the same bits: the one product chain G(a, b), the row statistics, the half-wave
// reductions of the mining, pos(c) and the group sums.  The rules are stated in include/xvec_hip.h; the chain and its error in
// the header of csrc/metric_loss.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "wave_reduce.h"
#include "xv_kernels.h"

// Every fused multiply-add of this file is written as fma(): where the rules round a product before it is used (u = x s,
// S_c - u_i, w sim + b) the compiler must not fuse it into the next operation.  A class of one row has S_c - u_i == 0 only so.
#pragma clang fp contract(off)

namespace xv {
namespace {

constexpr int kThreads = 512;
constexpr int kWaves = kThreads / 64;
constexpr int kPanelAnchors = 16;
constexpr int kQ = kThreads / kPanelAnchors;      // threads that share the positives of one anchor
static_assert(kQ == 32, "the mining takes one anchor per half-wave (ballot halves, xor shuffles below 32)");
constexpr int kNT = 4;                            // 16-column tiles a wave holds against one load of its 16 rows
constexpr int kPanelLdsRows = 1024;               // largest group whose panel lives in LDS
constexpr int kMaxRows = 4096;
constexpr int kMaxSlots = 1024;                   // workgroups of a slotted launch
constexpr double kEps = 1e-12;

typedef double d4 __attribute__((ext_vector_type(4)));

struct MetricArgs {
  const float* x;
  int64_t ldx;
  int d;
  int64_t num_groups;
  const int64_t* offsets;      // [G + 1], in the workspace
  const int32_t* panels;       // [P, 2] (group, first anchor), in the workspace
  int64_t num_panels;
  const int32_t* labels;
  double* scale;               // [rows], in the workspace
  double* nrm;                 // [rows]
  int64_t* aux;                // [rows]: triplets of the anchor (all), top1 == label (ge2e)
  int kind, head, m, squared, normalize, need_nrm;
  double margin, cosm, sinm, thr, w, b;
  double* row_loss;
  int64_t* row_count;
  int32_t* row_top1;
  double* group_loss;
  int64_t* group_count;
  double* slots;
  int64_t slot_doubles;
  int use_lds, max_rows, vec;  // vec: the rows of x are 16-byte aligned (float4 loads)
};

template <typename T>
struct Raw4 {
  T v[4];
};

// the four values k .. k + 3 of a row (zeros past d and for a row that is not there)
template <typename T>
__device__ __forceinline__ Raw4<T> load_raw(const T* __restrict__ row, bool ok, int k, int d, bool vec) {
  Raw4<T> r;
  if (sizeof(T) == 4 && vec && ok && k + 3 < d) {
    const float4 f = *reinterpret_cast<const float4*>(row + k);
    r.v[0] = (T)f.x;
    r.v[1] = (T)f.y;
    r.v[2] = (T)f.z;
    r.v[3] = (T)f.w;
  } else {
#pragma unroll
    for (int m = 0; m < 4; ++m) r.v[m] = (ok && k + m < d) ? row[k + m] : (T)0;
  }
  return r;
}

// acc[t] += A B_t^T over the columns [0, d), t < nv: A = the wave's 16 rows (this lane: a_row, scaled by sa), B_t = 16 rows each
// (this lane: b_row[t], scaled by sb[t]).  The one summation order of this file: see the header.
template <typename TB>
__device__ __forceinline__ void tile_products(const float* a_row, bool a_ok, double sa, bool avec, const TB* const (&b_row)[kNT],
                                              const bool (&b_ok)[kNT], const double (&sb)[kNT], bool bvec, int nv, int d,
                                              d4 (&acc)[kNT]) {
  const int kq = 4 * ((threadIdx.x & 63) >> 4);
  Raw4<float> ra = load_raw(a_row, a_ok, kq, d, avec);
  Raw4<TB> rb[kNT];
#pragma unroll
  for (int t = 0; t < kNT; ++t) rb[t] = load_raw(b_row[t], b_ok[t] && t < nv, kq, d, bvec);
  for (int k0 = 0; k0 < d; k0 += 16) {
    double da[4], db[kNT][4];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      da[m] = (double)ra.v[m] * sa;
#pragma unroll
      for (int t = 0; t < kNT; ++t) db[t][m] = (double)rb[t].v[m] * sb[t];
    }
    if (k0 + 16 < d) {
      ra = load_raw(a_row, a_ok, k0 + 16 + kq, d, avec);
#pragma unroll
      for (int t = 0; t < kNT; ++t) rb[t] = load_raw(b_row[t], b_ok[t] && t < nv, k0 + 16 + kq, d, bvec);
    }
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int t = 0; t < kNT; ++t)
        if (t < nv) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(da[m], db[t][m], acc[t], 0, 0, 0);
  }
}

// G(x_i, x_i) -> scale, then n = G(v, v) with v = x * scale: the chain of the panel kernel, 16 rows against themselves
__global__ __launch_bounds__(256) void row_stats_kernel(MetricArgs g, int64_t row_begin, int64_t row_end) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lr = lane & 15, lq = lane >> 4;
  const int64_t r = row_begin + ((int64_t)blockIdx.x * 4 + wave) * 16 + lr;
  const bool ok = r < row_end;
  const float* row = g.x + (ok ? r : row_begin) * g.ldx;
  double s = 1.0;
  for (int pass = 0; pass < (g.need_nrm ? 2 : 1); ++pass) {
    d4 acc = {0.0, 0.0, 0.0, 0.0};
    Raw4<float> raw = load_raw(row, ok, 4 * lq, g.d, g.vec);
    for (int k0 = 0; k0 < g.d; k0 += 16) {
      double v[4];
#pragma unroll
      for (int m = 0; m < 4; ++m) v[m] = (double)raw.v[m] * s;
      if (k0 + 16 < g.d) raw = load_raw(row, ok, k0 + 16 + 4 * lq, g.d, g.vec);
#pragma unroll
      for (int m = 0; m < 4; ++m) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(v[m], v[m], acc, 0, 0, 0);
    }
    // entry (i, i) is register i >> 2 of lane 16 (i & 3) + i
    const int e = lr >> 2;
    double dv = e == 0 ? acc[0] : e == 1 ? acc[1] : e == 2 ? acc[2] : acc[3];
    dv = __shfl(dv, 16 * (lr & 3) + lr);
    if (pass == 0) {
      s = g.normalize ? 1.0 / sqrt(fmax(dv, kEps)) : 1.0;
      if (ok && lq == 0) g.scale[r] = s;
    } else if (ok && lq == 0) {
      g.nrm[r] = dv;
    }
  }
}

// over the 32 lanes of a half-wave, the same bits in every lane of the half (a + b == b + a)
template <typename T>
__device__ __forceinline__ T half_sum(T v) {
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__device__ __forceinline__ double half_max(double v) {
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
  return v;
}

__device__ __forceinline__ double half_min(double v) {
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o));
  return v;
}

__device__ __forceinline__ double sgn(double v) { return (double)((v > 0.0) - (v < 0.0)); }

// the positive side of the angular triplet loss (model/loss.py:530-663): the margin function of the classifier heads
__device__ __forceinline__ double pos_value(double c, const MetricArgs& g) {
  if (g.head == XV_LOSS_ASOFTMAX) {
    if (g.m == 1) return c;
    const double s0 = sgn(c), c2 = c * c;
    if (g.m == 2) return 2.0 * s0 * c2 - 1.0;
    const double s3 = sgn(2.0 * c2 - 1.0) * s0, s4 = 2.0 * s0 + s3 - 3.0;
    return s3 * (8.0 * c2 * c2 - 8.0 * c2 + 1.0) + s4;
  }
  if (g.head == XV_LOSS_AMSOFTMAX) return c - g.margin;
  const double t = c * g.cosm - sqrt(1.0 - c * c) * g.sinm;
  return c <= g.thr ? -t - 2.0 : t;
}

__global__ __launch_bounds__(64) void finalize_kernel(MetricArgs g) {
  const int64_t grp = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (grp >= g.num_groups) return;
  const int64_t r0 = g.offsets[grp], r1 = g.offsets[grp + 1];
  double sum = 0.0;
  long long cnt = 0, aux = 0;
  for (int64_t r = r0; r < r1; ++r) {
    sum += g.row_loss[r];
    cnt += g.row_count[r];
    aux += g.aux[r];
  }
  double loss;
  if (g.kind == XV_METRIC_SEMIHARD) {
    loss = sum / fmax((double)cnt, 1e-16);
    aux = 0;
  } else if (g.kind == XV_METRIC_ANGULAR_ALL) {
    loss = sum / ((double)cnt + 1e-16);
  } else {
    loss = sum / (double)(r1 - r0);
    if (g.kind == XV_METRIC_ANGULAR_HARD) aux = 0;
  }
  g.group_loss[grp] = loss;
  g.group_count[2 * grp] = cnt;
  g.group_count[2 * grp + 1] = aux;
}

int64_t round256(int64_t v) { return (v + 255) / 256 * 256; }

}  // namespace
}  // namespace xv
