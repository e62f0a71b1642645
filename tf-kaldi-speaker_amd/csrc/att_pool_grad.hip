// Self-attentive pooling on tensors of the caller's own, forward and backward (model/pooling.py:150-218): the sibling of
// csrc/pool_grad.hip for pooling_type self_attention.  The pooling inside xv_forward is fused into the epilogues of the frozen
// key / value GEMMs and cannot be called on activations computed with the CURRENT weights; this file can.  The rule is stated in
// include/xvec_hip.h (xv_att_pool_forward, xv_att_pool_backward) and restated in float64 numpy, with the bounds below, in
// tests/helpers/ref_att_pool.py.
//
// Notation: H heads; dq = Dk / H with split_key, else Dk; dv = Dv / H with split_value, else Dv; P = H dv pooled columns, column
// p = h dv + d (head-major).  Head h reads the key columns kb + d, kb = split_key ? h dq : 0, and the value columns vb + d, vb =
// split_value ? h dv : 0.  u = 2^-24.  Every access is a 4-byte one, so any 4-byte aligned pointer and any legal pitch give the
// bits of the contiguous layout: there are no 16-byte accesses that would have to decline.
//
// Forward, three launches:
//  1. att_score_kernel, one wave per owned row: for each head, lane l runs ONE float32 fma chain over d = l, l + 64, l + 128, ...
//     from 0 (acc = fma(key, q, acc)); the 64 lane sums meet in an xor butterfly of float32 additions, distances 32 down to 1;
//     s = fl(scale * sum).  The order is a function of dq alone.  The raw scores are parked in weights_dev.
//     Bound: every product passes at most K = ceil(dq / 64) + 7 roundings, so |s^ - s| <= E = gamma_K |scale| sum_d |key q| +
//     (dq |scale| + 1) 2^-149, gamma_K = K u / (1 - K u).  The last term is the underflow term of fl(x) = x (1 + delta) + eta',
//     |eta'| <= 2^-150: an fma whose result is subnormal errs absolutely, whatever the size of its terms, so it counts per
//     OPERATION (dq fmas, then the scale), not per path as the relative part does; additions of subnormals are exact.
//  2. att_softmax_kernel, one workgroup of 256 threads per utterance, head after head: the max over the frames in float32 (exact),
//     then Z = sum_t exp(double(s_t) - double(max)) in double: thread i takes the frames i, i + 256, ... in ascending order, the 256
//     sums meet in LDS in a binary tree, strides 128 down to 1; w_t = float(exp(double(s_t) - double(max)) / Z), ONE rounding to
//     float32.  A function of n alone.
//     Bound: softmax(s^)_t / softmax(s)_t lies in [exp(-2 E), exp(2 E)], E the largest score bound of that (utterance, head); the
//     double steps (exp below 1 ulp, a sum of n <= 2^24 terms, one division) stay below 2^-27 relative, so
//     |w^ - w| <= w (exp(2 E)(1 + u + 2^-27) - 1) + 2^-149.
//  3. att_moments_kernel, one workgroup of 256 threads per (utterance, 64 pooled columns), the order of stat_pool_fwd_kernel:
//     thread = 16 slot + lane; slot s takes the frames s, s + 16, ... in ascending order into ONE float32 accumulator per column,
//     acc = fma(w, v, acc) from 0; the 16 slot sums meet in LDS in the binary tree of csrc/pool_grad.hip, neighbours first.  There is
//     no division: m is that sum.  Second sweep, same slots and tree: d = fl(v - m), e = fl(d d), acc = fma(w, e, acc).
//     std = sqrtf(var <= 1e-12f ? 1e-12f : var).  n = 0: m = 0, var = 0, std = sqrtf(1e-12f).  A function of n alone.
//     Bounds, against the float64 sums at the float32 w the kernel wrote, Kn = ceil(n / 16) + 4:
//     |m^ - m| <= gamma_Kn sum_t |w v| + n 2^-149 (n fmas, see above);  against the float64 sum about the float32 m the kernel
//     wrote, |var^ - var| <= gamma_(Kn + 3) var + (n + 2) 2^-149 (all terms are non-negative; n fmas, and squares that underflow
//     weigh sum_t w <= 1 + n u);
//     std is the correctly rounded root of the floored float32 var: |std^ - std| <= u std.
//
// Backward, a workspace and 3 + 2 (panels) launches; no floating-point atomics anywhere:
//  1. att_coef_kernel, one wave per (utterance, head): gvar = var > 1e-12f ? fl(gs / (2 std)) : 0 (2 std is exact) goes to the
//     workspace, and c = sum_d (gm m + gvar var) in double: lane l one fma chain over d = l, l + 64, ... (two fmas per d: gm m, then
//     gvar var), then the xor butterfly, distances 32 down to 1.
//  2. att_row_kernel, one wave per owned row; the wave finds its utterance by bisection in offsets_dev.  One pass over the value
//     row writes gvalue and sums gw[h] = sum_d (gm v + gvar (v - m)^2) in double in EXACTLY the order and instructions of c (lane
//     chains over d, two fmas per d, the same butterfly; v - m and its square are taken in double), so that for n = 1, where m = v
//     and gvar = 0 bit for bit, gw = c bit for bit and gscore is an exact zero.
//     gvalue: d = fl(v - m), t = fma(2 gvar, d, gm), out = fma(w_h, t, out) from 0, the heads in ascending order when the value is
//     not split (one head, out = fl(w t), when it is).  With Hs = split_value ? 1 : H,
//     |gvalue^ - gvalue| <= u (Hs + 4)(1 + 2^-20) sum_h w_h (|gm| + |2 gvar d|) + 2^-149 sum_h (1 + w_h |d|)
//     (per head: the division in gvar, the subtraction, the fma, then at most Hs accumulations; the last term: two fmas per head
//     that may underflow, and a gvar that does).
//     gscore = float(double(w) (gw - c)), one rounding: with A = sum_d (|gm v| + |gvar| (v - m)^2 + |gm m| + |gvar| var) and the
//     float32 gvar above (u relative to the rule's),
//     |gscore^ - gscore| <= Eg = u |gscore| + w (u sum_d |gvar| ((v - m)^2 + var) + (dv + 16) 2^-50 A) + 2^-149.
//     gkey: sg = fl(scale gscore); out = fma(sg, q, out) from 0 over the heads in ascending order when the key is not split, out =
//     fl(sg q) when it is.  With Hk = split_key ? 1 : H,
//     |gkey^ - gkey| <= sum_h |scale q| Eg_h (1 + 2^-20) + u (Hk + 2)(1 + 2^-20) sum_h |scale gscore_h q| + 2^-149 sum_h (1 + |q|)
//     (the last term: sg and the fma may underflow).
//     The float32 gscore also goes to the workspace, row r head h at r H + h.
//  3. att_gq_partial_kernel, one workgroup per (utterance, 64 query columns), the slots and the tree of the moments in double:
//     part[b][h, d] = sum_t double(gscore) double(key);  att_gq_final_kernel adds the utterances in ascending order in double into
//     a running sum and writes gquery = float(double(scale) sum) once.  The utterances are taken in panels of as many as the
//     workspace holds; the running sum makes the bits the same for every panel size.
//     |gquery^ - gquery| <= |scale| sum_t Eg_t |key| (1 + 2^-20) + u |gquery| + (rows + 32) 2^-50 |scale| sum_t |gscore key| + 2^-149.
#include "wave_reduce.h"
#include "xv_common.h"

namespace xv {

namespace {

constexpr int kApCols = 64;                   // columns per workgroup of the moments and of the gquery partials
constexpr int kApSlots = 16;                  // row slots of those workgroups
constexpr int kApWaves = 4;                   // waves, that is rows, per workgroup of the row kernels
constexpr int kApMaxHeads = 16;
constexpr float kApFloor = 1e-12f;            // VAR2STD_EPSILON of model/pooling.py

__device__ __forceinline__ float ap_wave_sum_f32(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = __fadd_rn(v, __shfl_xor(v, o, 64));
  return v;
}

template <class T>
__device__ __forceinline__ T ap_tree16(const T (*red)[kApCols], int c) {
  T q[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) q[i] = red[2 * i][c] + red[2 * i + 1][c];
#pragma unroll
  for (int i = 0; i < 4; ++i) q[i] = q[2 * i] + q[2 * i + 1];
  return (q[0] + q[1]) + (q[2] + q[3]);
}

// the owned rows [lo, hi) of the packed buffers: an offset the contract forbids reaches nothing outside [0, total_rows)
__device__ __forceinline__ void ap_range(const int32_t* __restrict__ offsets, int64_t batch, int64_t total_rows, int64_t* lo,
                                         int64_t* hi) {
  int64_t a = offsets[0], b = offsets[batch];
  if (a < 0) a = 0;
  if (b > total_rows) b = total_rows;
  *lo = a;
  *hi = b;
}

__device__ __forceinline__ void ap_utt(const int32_t* __restrict__ offsets, int64_t b, int64_t total_rows, int64_t* r0, int64_t* r1) {
  int64_t a = offsets[b], e = offsets[b + 1];
  if (a < 0) a = 0;
  if (e > total_rows) e = total_rows;
  if (e < a) e = a;
  *r0 = a;
  *r1 = e;
}

struct AttArgs {
  const float* key; int64_t ldk; int dq; int split_k;
  const float* value; int64_t ldv; int dv; int split_v;
  const float* query; int64_t ldq; int H; float scale;
  const int32_t* offsets; int64_t batch, total_rows;
  float* w; int64_t ldw;
  float* pooled; int64_t ldp;
  float* var; int64_t ldvar;
  int P;                                       // H dv
  const float* gp; int64_t ldgp;
  float* gkey; int64_t ldgk;
  float* gvalue; int64_t ldgv;
  float* gquery; int64_t ldgq;
  double* c;                                   // [batch, H]
  float* gvar;                                 // [batch, P]
  float* gscore;                               // [total_rows, H]
  double* run;                                 // [H dq]
  double* part;                                // [panel, H dq]
};

__global__ __launch_bounds__(256) void att_score_kernel(AttArgs p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t r = (int64_t)blockIdx.x * kApWaves + wave;
  int64_t lo, hi;
  ap_range(p.offsets, p.batch, p.total_rows, &lo, &hi);
  if (r < lo || r >= hi) return;
  const float* __restrict__ row = p.key + r * p.ldk;
  for (int h = 0; h < p.H; ++h) {
    const float* __restrict__ k = row + (p.split_k ? h * p.dq : 0);
    const float* __restrict__ q = p.query + h * p.ldq;
    float acc = 0.f;
#pragma unroll 4
    for (int d = lane; d < p.dq; d += 64) acc = fmaf(k[d], q[d], acc);
    const float s = __fmul_rn(p.scale, ap_wave_sum_f32(acc));
    if (lane == 0) p.w[r * p.ldw + h] = s;
  }
}

__global__ __launch_bounds__(256) void att_softmax_kernel(AttArgs p) {
  __shared__ float mx_s[256];
  __shared__ double z_s[256];
  const int tid = threadIdx.x;
  int64_t r0, r1;
  ap_utt(p.offsets, blockIdx.x, p.total_rows, &r0, &r1);
  const int64_t n = r1 - r0;
  if (n <= 0) return;
  for (int h = 0; h < p.H; ++h) {
    float* __restrict__ s = p.w + r0 * p.ldw + h;
    float mx = -INFINITY;
    for (int64_t t = tid; t < n; t += 256) mx = fmaxf(mx, s[t * p.ldw]);
    mx_s[tid] = mx;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if (tid < o) mx_s[tid] = fmaxf(mx_s[tid], mx_s[tid + o]);
      __syncthreads();
    }
    const double m = (double)mx_s[0];
    double z = 0.0;
    for (int64_t t = tid; t < n; t += 256) z += exp((double)s[t * p.ldw] - m);
    z_s[tid] = z;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if (tid < o) z_s[tid] = z_s[tid] + z_s[tid + o];
      __syncthreads();
    }
    const double Z = z_s[0];
    for (int64_t t = tid; t < n; t += 256) s[t * p.ldw] = (float)(exp((double)s[t * p.ldw] - m) / Z);
    __syncthreads();                           // mx_s and z_s are reused by the next head
  }
}

__global__ __launch_bounds__(256) void att_moments_kernel(AttArgs p, int nPb) {
  __shared__ float red[kApSlots][kApCols];
  __shared__ float mean_s[kApCols];
  const int64_t b = (int64_t)(blockIdx.x / (unsigned)nPb);
  const int p0 = (int)(blockIdx.x % (unsigned)nPb) * kApCols;
  const int lane = threadIdx.x & 15, slot = threadIdx.x >> 4;
  int64_t r0, r1;
  ap_utt(p.offsets, b, p.total_rows, &r0, &r1);
  bool ok[4];
  int vc[4], hc[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int pc = p0 + lane + 16 * k;
    ok[k] = pc < p.P;
    hc[k] = ok[k] ? pc / p.dv : 0;
    vc[k] = p.split_v ? pc : pc - hc[k] * p.dv;
  }
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
  for (int64_t r = r0 + slot; r < r1; r += kApSlots) {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (ok[k]) acc[k] = fmaf(p.w[r * p.ldw + hc[k]], p.value[r * p.ldv + vc[k]], acc[k]);
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) red[slot][lane + 16 * k] = acc[k];
  __syncthreads();
  float mean = 0.f;
  if (threadIdx.x < kApCols) {
    mean = ap_tree16<float>(red, threadIdx.x);
    mean_s[threadIdx.x] = mean;
  }
  __syncthreads();
  float m[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    m[k] = mean_s[lane + 16 * k];
    acc[k] = 0.f;
  }
#pragma unroll 4
  for (int64_t r = r0 + slot; r < r1; r += kApSlots) {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (ok[k]) {
        const float d = __fsub_rn(p.value[r * p.ldv + vc[k]], m[k]);
        acc[k] = fmaf(p.w[r * p.ldw + hc[k]], __fmul_rn(d, d), acc[k]);
      }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) red[slot][lane + 16 * k] = acc[k];      // every thread is past its reads of red: the sync above
  __syncthreads();
  const int pc = p0 + (int)threadIdx.x;
  if (threadIdx.x < kApCols && pc < p.P) {
    const float vv = ap_tree16<float>(red, threadIdx.x);
    p.pooled[b * p.ldp + pc] = mean;
    p.pooled[b * p.ldp + p.P + pc] = __fsqrt_rn(vv <= kApFloor ? kApFloor : vv);
    p.var[b * p.ldvar + pc] = vv;
  }
}

__global__ __launch_bounds__(256) void att_coef_kernel(AttArgs p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t idx = (int64_t)blockIdx.x * kApWaves + wave;
  if (idx >= p.batch * p.H) return;
  const int64_t b = idx / p.H;
  const int h = (int)(idx % p.H);
  const float* __restrict__ gp = p.gp + b * p.ldgp;
  const float* __restrict__ pl = p.pooled + b * p.ldp;
  double acc = 0.0;
  for (int d = lane; d < p.dv; d += 64) {
    const int pc = h * p.dv + d;
    const float vv = p.var[b * p.ldvar + pc];
    const float gv = vv > kApFloor ? __fdiv_rn(gp[p.P + pc], __fmul_rn(2.f, pl[p.P + pc])) : 0.f;
    acc = fma((double)gp[pc], (double)pl[pc], acc);
    acc = fma((double)gv, (double)vv, acc);
    p.gvar[b * p.P + pc] = gv;
  }
  acc = wave_sum_f64(acc);
  if (lane == 0) p.c[idx] = acc;
}

template <bool SPLIT_V>
__global__ __launch_bounds__(256) void att_row_kernel(AttArgs p) {
  __shared__ float sg_s[kApWaves][kApMaxHeads];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t r = (int64_t)blockIdx.x * kApWaves + wave;
  int64_t lo, hi;
  ap_range(p.offsets, p.batch, p.total_rows, &lo, &hi);
  if (r < lo || r >= hi) return;
  int64_t u = 0, top = p.batch - 1;            // the last utterance whose first row is <= r: it owns r
  while (u < top) {
    const int64_t mid = (u + top + 1) >> 1;
    if ((int64_t)p.offsets[mid] <= r) u = mid; else top = mid - 1;
  }
  const float* __restrict__ v = p.value + r * p.ldv;
  const float* __restrict__ gp = p.gp + u * p.ldgp;
  const float* __restrict__ pm = p.pooled + u * p.ldp;
  const float* __restrict__ gvar = p.gvar + u * p.P;
  const float* __restrict__ wr = p.w + r * p.ldw;
  float* __restrict__ gv = p.gvalue + r * p.ldgv;
  if (SPLIT_V) {
    for (int h = 0; h < p.H; ++h) {
      const float wh = wr[h];
      double acc = 0.0;
#pragma unroll 2
      for (int d = lane; d < p.dv; d += 64) {
        const int pc = h * p.dv + d;
        const float x = v[pc], m = pm[pc], gm = gp[pc], g = gvar[pc];
        const double dd = (double)x - (double)m;
        acc = fma((double)gm, (double)x, acc);
        acc = fma((double)g, dd * dd, acc);
        gv[pc] = __fmul_rn(wh, fmaf(__fmul_rn(2.f, g), __fsub_rn(x, m), gm));
      }
      acc = wave_sum_f64(acc);
      const float gs = (float)((double)wh * (acc - p.c[u * p.H + h]));
      sg_s[wave][h] = gs;                      // wave-uniform: every lane later reads what it wrote itself
      if (lane == 0) p.gscore[r * p.H + h] = gs;
    }
  } else {
    double acc[kApMaxHeads];
    float wh[kApMaxHeads];
#pragma unroll
    for (int h = 0; h < kApMaxHeads; ++h) {
      acc[h] = 0.0;
      wh[h] = h < p.H ? wr[h] : 0.f;
    }
    for (int d = lane; d < p.dv; d += 64) {
      const float x = v[d];
      float out = 0.f;
#pragma unroll
      for (int h = 0; h < kApMaxHeads; ++h)
        if (h < p.H) {
          const int pc = h * p.dv + d;
          const float m = pm[pc], gm = gp[pc], g = gvar[pc];
          const double dd = (double)x - (double)m;
          acc[h] = fma((double)gm, (double)x, acc[h]);
          acc[h] = fma((double)g, dd * dd, acc[h]);
          out = fmaf(wh[h], fmaf(__fmul_rn(2.f, g), __fsub_rn(x, m), gm), out);
        }
      gv[d] = out;
    }
#pragma unroll
    for (int h = 0; h < kApMaxHeads; ++h)
      if (h < p.H) {
        const double gw = wave_sum_f64(acc[h]);
        const float gs = (float)((double)wh[h] * (gw - p.c[u * p.H + h]));
        sg_s[wave][h] = gs;
        if (lane == 0) p.gscore[r * p.H + h] = gs;
      }
  }
  float* __restrict__ gk = p.gkey + r * p.ldgk;
  if (p.split_k) {
    for (int h = 0; h < p.H; ++h) {
      const float sg = __fmul_rn(p.scale, sg_s[wave][h]);
      const float* __restrict__ q = p.query + h * p.ldq;
      for (int d = lane; d < p.dq; d += 64) gk[h * p.dq + d] = __fmul_rn(sg, q[d]);
    }
  } else {
    for (int d = lane; d < p.dq; d += 64) {
      float out = 0.f;
      for (int h = 0; h < p.H; ++h) out = fmaf(__fmul_rn(p.scale, sg_s[wave][h]), p.query[h * p.ldq + d], out);
      gk[d] = out;
    }
  }
}

// part[b - b0][h dq + d] = sum_t gscore[t, h] key[t, kb + d] over the rows of utterance b, in double
__global__ __launch_bounds__(256) void att_gq_partial_kernel(AttArgs p, int64_t b0, int nQb) {
  __shared__ double red[kApSlots][kApCols];
  const int64_t bl = (int64_t)(blockIdx.x / (unsigned)nQb);
  const int c0 = (int)(blockIdx.x % (unsigned)nQb) * kApCols;
  const int lane = threadIdx.x & 15, slot = threadIdx.x >> 4;
  const int HQ = p.H * p.dq;
  int64_t r0, r1;
  ap_utt(p.offsets, b0 + bl, p.total_rows, &r0, &r1);
  bool ok[4];
  int kc[4], hc[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int qc = c0 + lane + 16 * k;
    ok[k] = qc < HQ;
    hc[k] = ok[k] ? qc / p.dq : 0;
    kc[k] = p.split_k ? qc : qc - hc[k] * p.dq;
  }
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
  for (int64_t r = r0 + slot; r < r1; r += kApSlots) {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (ok[k]) acc[k] = fma((double)p.gscore[r * p.H + hc[k]], (double)p.key[r * p.ldk + kc[k]], acc[k]);
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) red[slot][lane + 16 * k] = acc[k];
  __syncthreads();
  const int qc = c0 + (int)threadIdx.x;
  if (threadIdx.x < kApCols && qc < HQ) p.part[bl * HQ + qc] = ap_tree16<double>(red, threadIdx.x);
}

__global__ __launch_bounds__(256) void att_gq_final_kernel(AttArgs p, int64_t b0, int64_t nb) {
  const int HQ = p.H * p.dq;
  const int qc = (int)(blockIdx.x * 256 + threadIdx.x);
  if (qc >= HQ) return;
  double acc = b0 == 0 ? 0.0 : p.run[qc];
  for (int64_t b = 0; b < nb; ++b) acc += p.part[b * HQ + qc];
  p.run[qc] = acc;
  if (b0 + nb >= p.batch) p.gquery[(qc / p.dq) * p.ldgq + qc % p.dq] = (float)((double)p.scale * acc);
}

int64_t ap_round256(int64_t b) { return (b + 255) / 256 * 256; }

// bytes in front of the panel of partial sums
int64_t ap_fixed_bytes(int64_t batch, int64_t total_rows, int H, int dq, int P) {
  return ap_round256(batch * H * 8) + ap_round256(batch * P * 4) + ap_round256(total_rows * H * 4) + ap_round256((int64_t)H * dq * 8);
}

}  // namespace

int64_t att_pool_workspace_bytes(int64_t batch, int64_t total_rows, int H, int dq, int P, int64_t panel) {
  if (batch <= 0) return 0;
  return ap_fixed_bytes(batch, total_rows, H, dq, P) + ap_round256(panel * H * dq * 8);
}

hipError_t launch_att_pool_forward(const float* key, int64_t ldk, int dq, int split_k, const float* value, int64_t ldv, int dv,
                                   int split_v, const float* query, int64_t ldq, int H, float scale, const int32_t* offsets,
                                   int64_t batch, int64_t total_rows, float* w, int64_t ldw, float* pooled, int64_t ldp, float* var,
                                   int64_t ldvar, hipStream_t s) {
  if (batch <= 0) return hipSuccess;
  AttArgs a = {};
  a.key = key; a.ldk = ldk; a.dq = dq; a.split_k = split_k;
  a.value = value; a.ldv = ldv; a.dv = dv; a.split_v = split_v;
  a.query = query; a.ldq = ldq; a.H = H; a.scale = scale;
  a.offsets = offsets; a.batch = batch; a.total_rows = total_rows;
  a.w = w; a.ldw = ldw; a.pooled = pooled; a.ldp = ldp; a.var = var; a.ldvar = ldvar;
  a.P = H * dv;
  if (total_rows > 0) {
    hipLaunchKernelGGL(att_score_kernel, dim3((unsigned)((total_rows + kApWaves - 1) / kApWaves)), dim3(256), 0, s, a);
    hipLaunchKernelGGL(att_softmax_kernel, dim3((unsigned)batch), dim3(256), 0, s, a);
  }
  const int nPb = (a.P + kApCols - 1) / kApCols;
  hipLaunchKernelGGL(att_moments_kernel, dim3((unsigned)(batch * nPb)), dim3(256), 0, s, a, nPb);
  return hipGetLastError();
}

hipError_t launch_att_pool_backward(const float* gp, int64_t ldgp, const float* key, int64_t ldk, int dq, int split_k,
                                    const float* value, int64_t ldv, int dv, int split_v, const float* query, int64_t ldq, int H,
                                    float scale, const int32_t* offsets, int64_t batch, int64_t total_rows, const float* w,
                                    int64_t ldw, const float* pooled, int64_t ldp, const float* var, int64_t ldvar, float* gkey,
                                    int64_t ldgk, float* gvalue, int64_t ldgv, float* gquery, int64_t ldgq, void* ws, int64_t ws_bytes,
                                    hipStream_t s) {
  if (batch <= 0) return hipSuccess;
  AttArgs a = {};
  a.key = key; a.ldk = ldk; a.dq = dq; a.split_k = split_k;
  a.value = value; a.ldv = ldv; a.dv = dv; a.split_v = split_v;
  a.query = query; a.ldq = ldq; a.H = H; a.scale = scale;
  a.offsets = offsets; a.batch = batch; a.total_rows = total_rows;
  a.w = const_cast<float*>(w); a.ldw = ldw; a.pooled = const_cast<float*>(pooled); a.ldp = ldp;
  a.var = const_cast<float*>(var); a.ldvar = ldvar;
  a.P = H * dv;
  a.gp = gp; a.ldgp = ldgp; a.gkey = gkey; a.ldgk = ldgk; a.gvalue = gvalue; a.ldgv = ldgv; a.gquery = gquery; a.ldgq = ldgq;
  char* base = static_cast<char*>(ws);
  a.c = reinterpret_cast<double*>(base);
  base += ap_round256(batch * H * 8);
  a.gvar = reinterpret_cast<float*>(base);
  base += ap_round256(batch * a.P * 4);
  a.gscore = reinterpret_cast<float*>(base);
  base += ap_round256(total_rows * H * 4);
  a.run = reinterpret_cast<double*>(base);
  base += ap_round256((int64_t)H * dq * 8);
  a.part = reinterpret_cast<double*>(base);
  const int HQ = H * dq;
  int64_t panel = (ws_bytes - ap_fixed_bytes(batch, total_rows, H, dq, a.P)) / ((int64_t)HQ * 8);
  if (panel > batch) panel = batch;
  if (panel > 65536) panel = 65536;              // keeps every grid far below 2^31 workgroups; the bits do not depend on it
  if (panel < 1) return hipErrorInvalidValue;  // the C ABI checked ws_bytes
  hipLaunchKernelGGL(att_coef_kernel, dim3((unsigned)((batch * H + kApWaves - 1) / kApWaves)), dim3(256), 0, s, a);
  if (total_rows > 0) {
    const dim3 grid((unsigned)((total_rows + kApWaves - 1) / kApWaves));
    if (split_v)
      hipLaunchKernelGGL(att_row_kernel<true>, grid, dim3(256), 0, s, a);
    else
      hipLaunchKernelGGL(att_row_kernel<false>, grid, dim3(256), 0, s, a);
  }
  const int nQb = (HQ + kApCols - 1) / kApCols;
  for (int64_t b0 = 0; b0 < batch; b0 += panel) {
    const int64_t nb = batch - b0 < panel ? batch - b0 : panel;
    hipLaunchKernelGGL(att_gq_partial_kernel, dim3((unsigned)(nb * nQb)), dim3(256), 0, s, a, b0, nQb);
    hipLaunchKernelGGL(att_gq_final_kernel, dim3((unsigned)((HQ + 255) / 256)), dim3(256), 0, s, a, b0, nb);
  }
  return hipGetLastError();
}

}  // namespace xv
