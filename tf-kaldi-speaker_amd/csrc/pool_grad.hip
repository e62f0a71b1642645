// Statistics pooling on a tensor of the caller's own, forward and backward (model/pooling.py:27-52): what training the 1-tap
// frame layers behind the last multi-tap convolution (tdnn4 / tdnn5, tdnn8 .. tdnn10 of the extended TDNN) needs between
// xv_seg_forward / xv_seg_backward on the packed frames and on the pooled rows.  The pooling inside xv_forward lives in the
// epilogue of the last frozen GEMM and cannot be called on activations computed with the CURRENT weights; this file can.
// The rule is stated in include/xvec_hip.h (xv_stat_pool_forward, xv_stat_pool_backward) and restated in float64 numpy, with a
// float32 emulation of the order below, in tests/helpers/ref_pool_grad.py.
//
// Forward, one workgroup of 256 threads per (utterance, block of 64 channels), two sweeps over the utterance's n rows:
//  * thread t = 16 slot + lane.  Slot s (0 .. 15) takes the rows s, s + 16, s + 32, ... of the utterance in ascending order and
//    adds them to ONE float32 accumulator per channel, starting from 0 (fl(acc + x)).  A lane owns four channels of the block:
//    4 lane .. 4 lane + 3 with one 16-byte load where x, ldx and C allow (x 16-byte aligned, ldx and C multiples of 4), else
//    lane, lane + 16, lane + 32, lane + 48 with four 4-byte loads (still 64 contiguous bytes per row slot).  Which of the two a
//    channel meets changes no bit: its chain is the same.
//  * the 16 slot sums meet in LDS and one thread per channel adds them as a binary tree, neighbours first:
//    (((s0 + s1) + (s2 + s3)) + ((s4 + s5) + (s6 + s7))) + (((s8 + s9) + (s10 + s11)) + ((s12 + s13) + (s14 + s15))).
//  * m = S / float(n)  (a correctly rounded DIVISION, not a product with a rounded 1 / n).
//  * second sweep, same slots and the same tree: d = fl(x - m), acc = fma(d, d, acc) (one rounding);  v = Q / float(n);
//    std = sqrtf(v <= 1e-12f ? 1e-12f : v).  n = 0: m = 0, v = 0, std = sqrtf(1e-12f), no division.
//  So a channel's order is a function of n alone: 16 partial sums (k = 16 in the bars of tests/helpers/ref_pool.py: mean_bar,
//  var_bar, std_ratio) of at most ceil(n / 16) terms each, then a tree of depth 4.  Nothing depends on the utterance's position
//  in the packed buffer, on the batch around it, or on total_rows (which only clamps what a bad offset could reach).
//  A thread keeps its first 20 rows in registers between the sweeps (80 VGPRs): an utterance of up to 320 frames, every
//  training segment, is read from memory once with all its loads in flight together; later rows are read a second time from
//  L2 / MALL.  What is kept changes no bit.
//
// Backward, elementwise: gx_t = fma(b, d, a) with a = gm / float(n), b = live ? gs / (float(n) * std) : 0, d = fl(x_t - m),
// live = v > 1e-12f read from var_dev (the reference's floor mask is a constant to TensorFlow: a floored channel passes no
// gradient from std).  d var / d mean multiplies sum_t (x_t - m) = 0 and is dropped.  A workgroup takes 128 rows x (64 or 256)
// channels: wave w the rows 32 w .. 32 w + 31 of the chunk, a thread one channel (or four with 16-byte accesses, same
// condition as above with gx and ldgx).  A wave finds the utterance of its first row by bisection in offsets_dev and steps on
// when a row passes offsets[u + 1]; a, b and m are recomputed there, once per utterance met; inside an utterance eight rows are
// loaded before the first is stored.  No division per element, no
// workspace, one writer per element: the bits are a function of (x_t, m, std, v, gm, gs, n) alone.
//
// Error bound of the backward (u = 2^-24), against the float64 rule at the same float32 m, std, v, gm, gs.  Write a*, b*, d*
// for the exact values.  a^ = a* (1 + e1) (the division; float(n) is exact for n <= 2^24);  fl(float(n) std) = n std (1 + e2),
// b^ = b* (1 + e3) / (1 + e2);  d^ = d* (1 + e4);  gx^ = (b^ d^ + a^)(1 + e5), all |e_i| <= u.  Hence
//   gx^ - gx = a* e1 + b* d* (e3 + e4 - e2 + O(u^2)) + e5 (a^ + b^ d^),
//   |gx^ - gx| <= u |a| + 3 u |b d| + u (|a| + |b d|) + O(u^2) <= u (2 |a| + 4 |b d|)(1 + 2^-20) + 2^-149,
// where 1 + 2^-20 covers the products of two errors (at most 6 u (|a| + |b d|) u-terms) and 2^-149 a result that the fma
// rounds into the subnormal range.  A floored channel has b = 0 exactly and gx = a^ bit for bit.
#include "wave_reduce.h"
#include "xv_common.h"

namespace xv {

namespace {

constexpr int kPgChannels = 64;               // channels per forward workgroup
constexpr int kPgSlots = 16;                  // row slots per forward workgroup
constexpr int kPgRows = 32;                   // rows per wave of the backward
constexpr int kPgAheadB = 8;                  // rows a thread of the backward loads before it stores the first
constexpr int kPgKeep = 20;                   // rows per slot the forward keeps in registers between its two sweeps
constexpr int kPgAhead = 4;                   // rows of a slot (forward) or of a thread (backward) loaded before the first is used
constexpr float kPgFloor = 1e-12f;            // VAR_EPSILON of model/pooling.py

__device__ __forceinline__ float pg_tree16(const float (*red)[kPgChannels], int c) {
  float q[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) q[i] = __fadd_rn(red[2 * i][c], red[2 * i + 1][c]);
#pragma unroll
  for (int i = 0; i < 4; ++i) q[i] = __fadd_rn(q[2 * i], q[2 * i + 1]);
  return __fadd_rn(__fadd_rn(q[0], q[1]), __fadd_rn(q[2], q[3]));
}

// the four channels of a lane inside the 64-channel block: local index of channel k
template <bool VEC>
__device__ __forceinline__ int pg_local(int lane, int k) { return VEC ? 4 * lane + k : lane + 16 * k; }

template <bool VEC>
__device__ __forceinline__ void pg_load4(const float* __restrict__ row, int c0, int lane, int C, float v[4]) {
  if (VEC) {
    const int c = c0 + 4 * lane;
    if (c < C) {                               // C is a multiple of 4 here: the whole vector is inside
      const float4 q = *reinterpret_cast<const float4*>(row + c);
      v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
      v[0] = v[1] = v[2] = v[3] = 0.f;
    }
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int c = c0 + lane + 16 * k;
      v[k] = c < C ? row[c] : 0.f;
    }
  }
}

template <bool VEC>
__global__ __launch_bounds__(256) void stat_pool_fwd_kernel(const float* __restrict__ x, int64_t ldx, int C, int nCb,
                                                            const int32_t* __restrict__ offsets, int64_t total_rows,
                                                            float* __restrict__ pooled, int64_t ldp, float* __restrict__ var,
                                                            int64_t ldv) {
  __shared__ float red[kPgSlots][kPgChannels];
  __shared__ float mean_s[kPgChannels];
  const int64_t b = (int64_t)(blockIdx.x / (unsigned)nCb);
  const int c0 = (int)(blockIdx.x % (unsigned)nCb) * kPgChannels;
  const int lane = threadIdx.x & 15, slot = threadIdx.x >> 4;
  int64_t r0 = offsets[b], r1 = offsets[b + 1];
  if (r0 < 0) r0 = 0;                          // an offset the contract forbids reaches no row outside [0, total_rows)
  if (r1 > total_rows) r1 = total_rows;
  const int n = r1 > r0 ? (int)(r1 - r0) : 0;
  r1 = r0 + n;

  // The first kPgKeep rows of a slot stay in registers for the second sweep: an utterance of up to 16 kPgKeep = 320 frames is
  // read from memory ONCE, and all of its loads are in flight together.  Later rows are read again, kPgAhead at a time.  Rows
  // are added in ascending order either way, so the chain is the one stated above.
  float acc[4] = {0.f, 0.f, 0.f, 0.f}, v[4], w[kPgAhead][4], keep[kPgKeep][4];
#pragma unroll
  for (int i = 0; i < kPgKeep; ++i) {
    const int64_t rr = r0 + slot + (int64_t)i * kPgSlots;
    if (rr < r1) pg_load4<VEC>(x + rr * ldx, c0, lane, C, keep[i]);
  }
#pragma unroll
  for (int i = 0; i < kPgKeep; ++i)
    if (r0 + slot + (int64_t)i * kPgSlots < r1) {
#pragma unroll
      for (int k = 0; k < 4; ++k) acc[k] = __fadd_rn(acc[k], keep[i][k]);
    }
  int64_t r = r0 + slot + (int64_t)kPgKeep * kPgSlots;
  for (; r + (kPgAhead - 1) * kPgSlots < r1; r += kPgAhead * kPgSlots) {
#pragma unroll
    for (int i = 0; i < kPgAhead; ++i) pg_load4<VEC>(x + (r + i * kPgSlots) * ldx, c0, lane, C, w[i]);
#pragma unroll
    for (int i = 0; i < kPgAhead; ++i)
#pragma unroll
      for (int k = 0; k < 4; ++k) acc[k] = __fadd_rn(acc[k], w[i][k]);
  }
  for (; r < r1; r += kPgSlots) {
    pg_load4<VEC>(x + r * ldx, c0, lane, C, v);
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[k] = __fadd_rn(acc[k], v[k]);
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) red[slot][pg_local<VEC>(lane, k)] = acc[k];
  __syncthreads();
  float mean = 0.f;
  if (threadIdx.x < kPgChannels) {
    const float s = pg_tree16(red, threadIdx.x);
    mean = n > 0 ? __fdiv_rn(s, (float)n) : 0.f;
    mean_s[threadIdx.x] = mean;
  }
  __syncthreads();

  float m[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    m[k] = mean_s[pg_local<VEC>(lane, k)];
    acc[k] = 0.f;
  }
#pragma unroll
  for (int i = 0; i < kPgKeep; ++i)
    if (r0 + slot + (int64_t)i * kPgSlots < r1) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float d = __fsub_rn(keep[i][k], m[k]);
        acc[k] = fmaf(d, d, acc[k]);
      }
    }
  r = r0 + slot + (int64_t)kPgKeep * kPgSlots;
  for (; r + (kPgAhead - 1) * kPgSlots < r1; r += kPgAhead * kPgSlots) {
#pragma unroll
    for (int i = 0; i < kPgAhead; ++i) pg_load4<VEC>(x + (r + i * kPgSlots) * ldx, c0, lane, C, w[i]);
#pragma unroll
    for (int i = 0; i < kPgAhead; ++i)
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float d = __fsub_rn(w[i][k], m[k]);
        acc[k] = fmaf(d, d, acc[k]);
      }
  }
  for (; r < r1; r += kPgSlots) {
    pg_load4<VEC>(x + r * ldx, c0, lane, C, v);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float d = __fsub_rn(v[k], m[k]);
      acc[k] = fmaf(d, d, acc[k]);
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) red[slot][pg_local<VEC>(lane, k)] = acc[k];      // every thread is past its reads of red: the sync above
  __syncthreads();
  const int c = c0 + (int)threadIdx.x;
  if (threadIdx.x < kPgChannels && c < C) {
    const float q = pg_tree16(red, threadIdx.x);
    const float vv = n > 0 ? __fdiv_rn(q, (float)n) : 0.f;
    pooled[b * ldp + c] = mean;
    pooled[b * ldp + C + c] = __fsqrt_rn(vv <= kPgFloor ? kPgFloor : vv);
    var[b * ldv + c] = vv;
  }
}

struct PoolBwdArgs {
  const float* gp; int64_t ldgp;
  const float* x; int64_t ldx;
  int C;
  const int32_t* offsets; int64_t batch, total_rows;
  const float* pooled; int64_t ldp;
  const float* var; int64_t ldv;
  float* gx; int64_t ldgx;
};

__device__ __forceinline__ float4 pg_gx4(const float4 q, const float* a, const float* b, const float* m) {
  float4 o;
  o.x = fmaf(b[0], __fsub_rn(q.x, m[0]), a[0]);
  o.y = fmaf(b[1], __fsub_rn(q.y, m[1]), a[1]);
  o.z = fmaf(b[2], __fsub_rn(q.z, m[2]), a[2]);
  o.w = fmaf(b[3], __fsub_rn(q.w, m[3]), a[3]);
  return o;
}

template <bool VEC>
__global__ __launch_bounds__(256) void stat_pool_bwd_kernel(PoolBwdArgs p) {
  constexpr int V = VEC ? 4 : 1;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int c = ((int)blockIdx.y * 64 + tx) * V;
  int64_t ra = ((int64_t)blockIdx.x * 4 + ty) * kPgRows, rb = ra + kPgRows;
  int64_t lo = p.offsets[0], hi = p.offsets[p.batch];
  if (lo < 0) lo = 0;
  if (hi > p.total_rows) hi = p.total_rows;
  if (ra < lo) ra = lo;
  if (rb > hi) rb = hi;
  if (ra >= rb || c >= p.C) return;

  int64_t u = 0, top = p.batch - 1;            // the last utterance whose first row is <= ra
  while (u < top) {
    const int64_t mid = (u + top + 1) >> 1;
    if ((int64_t)p.offsets[mid] <= ra) u = mid; else top = mid - 1;
  }
  float a[4], b[4], m[4];
  int64_t r = ra;
  while (r < rb) {
    while ((int64_t)p.offsets[u + 1] <= r) ++u;            // r < offsets[batch]: u stays below batch
    const int64_t last = p.offsets[u + 1];
    const int64_t end = last < rb ? last : rb;              // the rows of utterance u in this wave's chunk
    const float fn = (float)(last - (int64_t)p.offsets[u]);
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const float gm = p.gp[u * p.ldgp + c + k], gs = p.gp[u * p.ldgp + p.C + c + k];
      const float sd = p.pooled[u * p.ldp + p.C + c + k];
      m[k] = p.pooled[u * p.ldp + c + k];
      a[k] = __fdiv_rn(gm, fn);
      b[k] = p.var[u * p.ldv + c + k] > kPgFloor ? __fdiv_rn(gs, __fmul_rn(fn, sd)) : 0.f;
    }
    if (VEC) {
      for (; r + kPgAheadB <= end; r += kPgAheadB) {
        float4 q[kPgAheadB];
#pragma unroll
        for (int i = 0; i < kPgAheadB; ++i) q[i] = *reinterpret_cast<const float4*>(p.x + (r + i) * p.ldx + c);
#pragma unroll
        for (int i = 0; i < kPgAheadB; ++i) *reinterpret_cast<float4*>(p.gx + (r + i) * p.ldgx + c) = pg_gx4(q[i], a, b, m);
      }
      for (; r < end; ++r)
        *reinterpret_cast<float4*>(p.gx + r * p.ldgx + c) = pg_gx4(*reinterpret_cast<const float4*>(p.x + r * p.ldx + c), a, b, m);
    } else {
      for (; r + kPgAheadB <= end; r += kPgAheadB) {
        float q[kPgAheadB];
#pragma unroll
        for (int i = 0; i < kPgAheadB; ++i) q[i] = p.x[(r + i) * p.ldx + c];
#pragma unroll
        for (int i = 0; i < kPgAheadB; ++i) p.gx[(r + i) * p.ldgx + c] = fmaf(b[0], __fsub_rn(q[i], m[0]), a[0]);
      }
      for (; r < end; ++r) p.gx[r * p.ldgx + c] = fmaf(b[0], __fsub_rn(p.x[r * p.ldx + c], m[0]), a[0]);
    }
  }
}

}  // namespace

hipError_t launch_stat_pool_forward(const float* x, int64_t ldx, int C, const int32_t* offsets, int64_t batch, int64_t total_rows,
                                    float* pooled, int64_t ldp, float* var, int64_t ldv, hipStream_t s) {
  if (batch <= 0) return hipSuccess;
  const int nCb = (C + kPgChannels - 1) / kPgChannels;
  const dim3 grid((unsigned)(batch * nCb));
  if (aligned16(x) && ldx % 4 == 0 && C % 4 == 0)
    hipLaunchKernelGGL(stat_pool_fwd_kernel<true>, grid, dim3(256), 0, s, x, ldx, C, nCb, offsets, total_rows, pooled, ldp, var, ldv);
  else
    hipLaunchKernelGGL(stat_pool_fwd_kernel<false>, grid, dim3(256), 0, s, x, ldx, C, nCb, offsets, total_rows, pooled, ldp, var, ldv);
  return hipGetLastError();
}

hipError_t launch_stat_pool_backward(const float* gp, int64_t ldgp, const float* x, int64_t ldx, int C, const int32_t* offsets,
                                     int64_t batch, int64_t total_rows, const float* pooled, int64_t ldp, const float* var,
                                     int64_t ldv, float* gx, int64_t ldgx, hipStream_t s) {
  if (batch <= 0 || total_rows <= 0) return hipSuccess;
  PoolBwdArgs a = {gp, ldgp, x, ldx, C, offsets, batch, total_rows, pooled, ldp, var, ldv, gx, ldgx};
  const bool vec = aligned16(x) && aligned16(gx) && ldx % 4 == 0 && ldgx % 4 == 0 && C % 4 == 0;
  const int per = 64 * (vec ? 4 : 1);
  const dim3 grid((unsigned)((total_rows + 4 * kPgRows - 1) / (4 * kPgRows)), (unsigned)((C + per - 1) / per));
  if (vec)
    hipLaunchKernelGGL(stat_pool_bwd_kernel<true>, grid, dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL(stat_pool_bwd_kernel<false>, grid, dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace xv
