// Batch norm in TRAINING mode behind the stored product z of a trained layer: the batch statistics, h and y, the moving-average
// update, and the gradient through the statistics.  z [n, N] is what xv_seg_forward / xv_tconv_forward store when they are called
// without batch norm and with XV_SEG_ACT_NONE; the gz of the backward goes back into xv_seg_backward / xv_tconv_backward (again
// without batch norm, XV_SEG_ACT_NONE) as their gy, whose mask kernels pass it through and give gbias, gw and gx by their own
// rules.  The rule is stated in include/xvec_hip.h (xv_bn_batch_forward, xv_bn_batch_backward) and restated in float64 numpy in
// tests/helpers/ref_bn_batch.py; torch.autograd of batch_norm(training=True, eps=1e-3) + relu / leaky_relu(0.2) gives the same
// numbers (tests/test_bn_batch_host.py).  Every line behind the statistics is csrc/layer_lines.h's (bn_r, bn_h, act_y, act_grad,
// kBnEps): forward, backward and the inference path of the other operators run the same instructions on the stored z.
//
//  forward    S1_j = sum_i double(z_ij),  mu_j = float(S1_j / n);   S2_j = sum_i (double(z_ij) - double(mu_j))^2,  v_j = float(S2_j / n)
//             (two sweeps, the second about the ROUNDED mean);  r_j = bn_r(v_j),  s_j = gamma_j * r_j,  h_ij = bn_h(z_ij, s_j, mu_j,
//             beta_j),  y_ij = act_y(h_ij).   d = float(1 - double(momentum)),  f = float(double(n) / double(max(n - 1, 1))),
//             v'_j = bessel ? v_j * f : v_j;  moving_mean_j -= (moving_mean_j - mu_j) * d,  moving_variance_j -= (moving_variance_j -
//             v'_j) * d, each operation rounded to float32 on its own (tf assign_moving_average without zero_debias).
//  backward   a_ij = act_grad(gy_ij, h_ij) with the forward's bits of h,  xh_ij = double(r_j) * (double(z_ij) - double(mu_j)),
//             A_j = sum_i double(a_ij),  G_j = sum_i double(a_ij) * xh_ij,  gbeta_j = float(A_j),  ggamma_j = float(G_j),
//             gz_ij = float(double(s_j) * ((double(a_ij) - A_j / n) - xh_ij * (G_j / n)))    (one rounding, the unrounded sums).
//
// Launches.  bn_sweep_kernel<MODE> is the column-sum kernel, in the order of tc_mask_kernel (csrc/tconv_grad.hip): the rows are cut
// into R slices of rows_per_slice rows (bn_slices: the rule of tc_slices, a function of n alone: max(1024, ceil(n / 64) rounded
// up to 64) rows, so n = 1025 is the first with two slices); a workgroup takes 32 columns of one slice, reads along the rows (a
// half wave per row) into an LDS tile of 64 rows, then lane l of the wave that owns column j adds the rows i = l (mod 64) in
// ascending order to its doubles, wave_sum_f64 closes the slice.  bn_mean_kernel / bn_var_kernel / bn_grad_kernel, one thread
// per column, add the R slice sums in ascending order in double and round once.  bn_apply_kernel / bn_gz_kernel are elementwise.
// Forward: sweep (z), mean, sweep (z), var + moving update, apply (z -> y): three reads of z, one write.  Backward: sweep (gy,
// z), grad, gz (gy, z -> gz): two reads of gy and z, one write.  All loads and stores are scalar float32 (a half wave or a wave
// reads consecutive columns of a row), so any 4-byte aligned pointer and any leading dimension >= N take the same path and give
// the same bits; there is no 16-byte path to fall back from.  Every double expression, and the three float32 operations of each
// moving update, are plain operators under `#pragma clang fp contract(off)`: hipcc's __fmul_rn / __fsub_rn are `x * y` and `x - y`
// compiled with contraction on, and a product of theirs that feeds a difference becomes one fma.  One writer per element, a fixed order, no floating-point atomics, nothing read that this call did not write;
// nothing of the workspace depends on ws_bytes (xv_bn_batch_workspace_min and xv_bn_batch_workspace agree).
//
// Error bound (u = 2^-24; checked per element in tests/test_gpu_bn_batch.py, restated in ref_bn_batch.bounds).  |.| of the float64
// oracle's values, the oracle evaluating the rule above in float64 (with the same float32 d and f); Bz is the caller's bound of
// z_ij (0 when the oracle starts from the device's own z); t = 2^-53 (n + 64) covers a double sum of n terms in any order, the
// roundings of its terms and the division by n.  mean_i is the mean over the rows of column j.
//   mu_j:   Bmu = mean_i Bz + t mean_i |z_ij| + u |mu_j|
//   v_j:    for any centre c, sum_i (z_i + e_i - c)^2 = n v + 2 sum_i (z_i - mu) e_i + sum_i (e_i - (c - mu))^2, because
//           sum_i (z_i - mu) = 0: the rounding of the mean enters in second order only (which is why the second sweep may run
//           about the rounded mean, and why a one-sweep E[z^2] - mu^2 would not do: there the roundings of z^2 ~ mu^2 enter in
//           first order).  Q = mean_i (2 |z_ij - mu_j| Bz + (Bz + Bmu)^2),   Bv = Q + (u + t) (v_j + Q)
//   r_j:    Br = 0.5 (max(v_j - Bv, 0) + kBnEps)^-1.5 Bv + 1.01 u r_j.   |dr/dv| = 0.5 (v + eps)^-1.5 is largest where v is far
//           below kBnEps (15811 at v = 0) and still 0.18 of that at v = 2 kBnEps: there r AMPLIFIES the absolute error of v, and
//           everything behind r carries it.  (v and the computed v are both >= 0, so the derivative on the whole interval between
//           them is at most the one at max(v - Bv, 0).)
//   s_j:    Bs = |gamma_j| Br + u (|s_j| + |gamma_j| Br)
//   h_ij:   Bd = Bz + Bmu + u (|z_ij - mu_j| + Bz + Bmu),   E = |s_j| Bd + Bs (|z_ij - mu_j| + Bd),   Bh = E + u (|h_ij| + E)
//   y_ij:   By = Bh + 2 u |y_ij|      (the sign of h is the oracle's wherever |h| > Bh, which the cases guarantee with a factor of
//           64, or where h = 0 exactly in both: gamma_j = beta_j = 0)
//   moving_mean_j:      1.01 d Bmu + 2.01 u d |mm_j - mu_j| + u |mm'_j|           (subtract, multiply, subtract: one u each)
//   moving_variance_j:  Bv' = f Bv + 1.01 u v'_j (Bv' = Bv without bessel);  1.01 d Bv' + 2.01 u d |mv_j - v'_j| + u |mv'_j|
//   a_ij:   Ba = 2 u |a_ij| (leaky ReLU; 0 for ReLU and none, where a is gy or 0 exactly)
//   xh_ij:  Bx = Br (|z_ij - mu_j| + Bz + Bmu) + r_j (Bz + Bmu)            (the device's r and mu are the forward's rounded ones)
//   A_j:    BA = sum_i Ba + t sum_i |a_ij|;                                 gbeta_j:  BA + u |A_j|
//   G_j:    BG = sum_i (Ba (|xh_ij| + Bx) + |a_ij| Bx) + 1.01 t sum_i |a_ij| (|xh_ij| + Bx);        ggamma_j: BG + u |G_j|
//   gz_ij:  p = a - A / n - xh G / n,   Bp = Ba + BA / n + (Bx (|G_j| + BG) + |xh_ij| BG) / n + t (|a_ij| + |A_j| / n + |xh_ij G_j| / n),
//           Eg = |s_j| Bp + Bs (|p_ij| + Bp),   Bgz = Eg + u (|gz_ij| + Eg)      (p cancels; its bound is in the absolute terms)
#include "layer_lines.h"

namespace xv {

namespace {

constexpr int kBnCols = 32;                   // columns per workgroup of bn_sweep_kernel, 8 per wave
constexpr int kBnMaxSlices = 64;
constexpr int kBnApplyCols = 64;              // bn_apply_kernel, bn_gz_kernel: a wave per row of 64 columns, 4 rows per pass
constexpr int kBnApplyRows = 16;              // rows per workgroup

enum { BN_SUM = 0, BN_SQ = 1, BN_GRAD = 2 };

inline int64_t bn_up(int64_t v, int64_t m) { return (v + m - 1) / m * m; }

// the row slices of every column sum: a function of n alone (the rule of tc_slices, csrc/tconv_grad.hip)
void bn_slices(int64_t n, int64_t* rows_per_slice, int* slices) {
  int64_t rows = bn_up((n + kBnMaxSlices - 1) / kBnMaxSlices, 64);
  if (rows < 1024) rows = 1024;
  *rows_per_slice = rows;
  *slices = (int)((n + rows - 1) / rows);
}

struct BnSweepArgs {
  const float* z; int64_t ldz;
  const float* gy; int64_t ldgy;              // BN_GRAD
  int64_t n, rows_per_slice;
  int N, slices;
  const float *mean, *var, *gamma, *beta;     // BN_SQ: mean; BN_GRAD: all four
  int act;
  double* part;                               // [2][N][slices]; BN_SUM and BN_SQ use the first plane
};

// BN_SUM: sum_i double(z).  BN_SQ: sum_i (double(z) - double(mu))^2.  BN_GRAD: sum_i double(a) and sum_i double(a) xh.
template <int MODE>
__global__ __launch_bounds__(256) void bn_sweep_kernel(BnSweepArgs p) {
#pragma clang fp contract(off)
  constexpr int CW = kBnCols / 4;
  __shared__ float tz[64][kBnCols + 1], ta[MODE == BN_GRAD ? 64 : 1][kBnCols + 1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j0 = (int)blockIdx.x * kBnCols;
  const int64_t row0 = (int64_t)blockIdx.y * p.rows_per_slice;
  const int64_t row1 = row0 + p.rows_per_slice < p.n ? row0 + p.rows_per_slice : p.n;
  // phase 1 reads along the rows: a half wave takes 32 columns of one row
  const int c1 = lane & 31, rsub = 2 * wave + (lane >> 5);
  const int jc = j0 + c1;
  const bool jok = jc < p.N;
  float s1 = 0.f, mu1 = 0.f, beta1 = 0.f;
  if (MODE == BN_GRAD && jok) {
    s1 = __fmul_rn(p.gamma[jc], lines::bn_r(p.var[jc]));
    mu1 = p.mean[jc];
    beta1 = p.beta[jc];
  }
  // phase 2 sums along the columns: wave w owns the columns j0 + 8 w + c, lane = row of the 64-row chunk
  double mu2[CW], r2[CW], s0[CW], sg[CW];
#pragma unroll
  for (int c = 0; c < CW; ++c) {
    const int j = j0 + CW * wave + c;
    mu2[c] = r2[c] = s0[c] = sg[c] = 0.0;
    if (j < p.N && MODE != BN_SUM) mu2[c] = (double)p.mean[j];
    if (j < p.N && MODE == BN_GRAD) r2[c] = (double)lines::bn_r(p.var[j]);
  }
  for (int64_t i0 = row0; i0 < row1; i0 += 64) {
    for (int rl = rsub; rl < 64; rl += 8) {
      const int64_t i = i0 + rl;
      float a = 0.f, z = 0.f;
      if (i < row1 && jok) {
        z = p.z[i * p.ldz + jc];
        if (MODE == BN_GRAD) a = lines::act_grad(p.gy[i * p.ldgy + jc], lines::bn_h(z, s1, mu1, beta1), p.act);
      }
      tz[rl][c1] = z;
      if (MODE == BN_GRAD) ta[rl][c1] = a;
    }
    __syncthreads();
    if (i0 + lane < row1) {
#pragma unroll
      for (int c = 0; c < CW; ++c) {
        const int cl = CW * wave + c;
        if (j0 + cl < p.N) {
          const double z = (double)tz[lane][cl];
          if (MODE == BN_SUM) {
            s0[c] = s0[c] + z;
          } else if (MODE == BN_SQ) {
            const double d = z - mu2[c];
            const double q = d * d;
            s0[c] = s0[c] + q;
          } else {
            const double a = (double)ta[lane][cl];
            const double d = z - mu2[c];
            const double xh = r2[c] * d;
            const double q = a * xh;
            s0[c] = s0[c] + a;
            sg[c] = sg[c] + q;
          }
        }
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int c = 0; c < CW; ++c) {
    const int j = j0 + CW * wave + c;
    if (j >= p.N) continue;                                       // uniform over the wave
    const double a = wave_sum_f64(s0[c]);
    if (lane == 0) p.part[((int64_t)0 * p.N + j) * p.slices + blockIdx.y] = a;
    if (MODE == BN_GRAD) {
      const double g = wave_sum_f64(sg[c]);
      if (lane == 0) p.part[((int64_t)1 * p.N + j) * p.slices + blockIdx.y] = g;
    }
  }
}

__device__ __forceinline__ double bn_slice_sum(const double* __restrict__ part, int64_t plane, int N, int slices, int j) {
#pragma clang fp contract(off)
  double s = 0.0;
  for (int i = 0; i < slices; ++i) s = s + part[(plane * N + j) * slices + i];
  return s;
}

__global__ __launch_bounds__(256) void bn_mean_kernel(const double* __restrict__ part, int N, int slices, int64_t n,
                                                      float* __restrict__ mean) {
#pragma clang fp contract(off)
  const int j = (int)(blockIdx.x * 256 + threadIdx.x);
  if (j >= N) return;
  mean[j] = (float)(bn_slice_sum(part, 0, N, slices, j) / (double)n);
}

// v, then the two moving averages in place (mm, mv: both or neither)
__global__ __launch_bounds__(256) void bn_var_kernel(const double* __restrict__ part, int N, int slices, int64_t n,
                                                     const float* __restrict__ mean, float* __restrict__ var, float d, float f,
                                                     int bessel, float* __restrict__ mm, float* __restrict__ mv) {
#pragma clang fp contract(off)
  const int j = (int)(blockIdx.x * 256 + threadIdx.x);
  if (j >= N) return;
  const float v = (float)(bn_slice_sum(part, 0, N, slices, j) / (double)n);
  var[j] = v;
  if (!mm) return;
  // plain operators under contract(off): hipcc's __fmul_rn / __fsub_rn are x * y and x - y, which it would fuse into one fma
  const float vb = bessel ? v * f : v;
  const float m0 = mm[j], v0 = mv[j];
  const float dm = m0 - mean[j], dv = v0 - vb;
  const float pm = dm * d, pv = dv * d;
  mm[j] = m0 - pm;
  mv[j] = v0 - pv;
}

// gbeta, ggamma and the unrounded sums [2][N] for bn_gz_kernel
__global__ __launch_bounds__(256) void bn_grad_kernel(const double* __restrict__ part, int N, int slices, float* __restrict__ gbeta,
                                                      float* __restrict__ ggamma, double* __restrict__ sums) {
  const int j = (int)(blockIdx.x * 256 + threadIdx.x);
  if (j >= N) return;
  const double a = bn_slice_sum(part, 0, N, slices, j), g = bn_slice_sum(part, 1, N, slices, j);
  gbeta[j] = (float)a;
  ggamma[j] = (float)g;
  sums[j] = a;
  sums[N + j] = g;
}

struct BnApplyArgs {
  const float* z; int64_t ldz;
  const float* gy; int64_t ldgy;              // bn_gz_kernel
  int64_t n;
  int N;
  const float *mean, *var, *gamma, *beta;
  int act;
  const double* sums;                         // bn_gz_kernel: A [N], G [N]
  float* out; int64_t ldo;                    // y or gz
};

// y = act_y(bn_h(z)) (GZ = false) or gz (GZ = true): a wave takes 64 columns of one row, a workgroup 16 rows
template <bool GZ>
__global__ __launch_bounds__(256) void bn_apply_kernel(BnApplyArgs p) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = (int)blockIdx.y * kBnApplyCols + lane;
  if (j >= p.N) return;
  const float mu = p.mean[j], beta = p.beta[j];
  const float r = lines::bn_r(p.var[j]);
  const float s = __fmul_rn(p.gamma[j], r);
  double an = 0.0, gn = 0.0;
  if (GZ) {
    an = p.sums[j] / (double)p.n;
    gn = p.sums[p.N + j] / (double)p.n;
  }
  const int64_t i0 = (int64_t)blockIdx.x * kBnApplyRows;
#pragma unroll
  for (int q = 0; q < kBnApplyRows / 4; ++q) {
    const int64_t i = i0 + 4 * q + wave;
    if (i >= p.n) break;
    const float z = p.z[i * p.ldz + j];
    const float h = lines::bn_h(z, s, mu, beta);
    if (!GZ) {
      p.out[i * p.ldo + j] = lines::act_y(h, p.act);
    } else {
      const double a = (double)lines::act_grad(p.gy[i * p.ldgy + j], h, p.act);
      const double d = (double)z - (double)mu;
      const double xh = (double)r * d;
      const double t1 = a - an;
      const double t2 = xh * gn;
      const double t3 = t1 - t2;
      p.out[i * p.ldo + j] = (float)((double)s * t3);
    }
  }
}

struct BnLayout {
  int64_t part, sums, total;                  // byte offsets
};

BnLayout bn_layout(int64_t n, int N) {
  int64_t rows;
  int slices;
  bn_slices(n, &rows, &slices);
  BnLayout L;
  int64_t o = 0;
  L.part = o; o += bn_up((int64_t)8 * 2 * N * slices, 256);
  L.sums = o; o += bn_up((int64_t)8 * 2 * N, 256);
  L.total = o;
  return L;
}

template <int MODE>
hipError_t bn_sweep(BnSweepArgs a, hipStream_t s) {
  hipLaunchKernelGGL(bn_sweep_kernel<MODE>, dim3((unsigned)((a.N + kBnCols - 1) / kBnCols), (unsigned)a.slices), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace

int64_t bn_batch_workspace_bytes(int64_t n, int N) {
  if (n <= 0 || N <= 0) return 0;
  return bn_layout(n, N).total;
}

hipError_t launch_bn_batch_forward(const float* z, int64_t ldz, int64_t n, int N, const float* gamma, const float* beta, int act,
                                   double momentum, int bessel, float* mm, float* mv, float* y, int64_t ldy, float* mean, float* var,
                                   void* ws, hipStream_t s) {
  const BnLayout L = bn_layout(n, N);
  double* part = reinterpret_cast<double*>(static_cast<char*>(ws) + L.part);
  const unsigned cols = (unsigned)((N + 255) / 256);
  BnSweepArgs a = {};
  a.z = z; a.ldz = ldz; a.n = n; a.N = N; a.part = part;
  bn_slices(n, &a.rows_per_slice, &a.slices);
  hipError_t e;
  if ((e = bn_sweep<BN_SUM>(a, s)) != hipSuccess) return e;
  hipLaunchKernelGGL(bn_mean_kernel, dim3(cols), dim3(256), 0, s, (const double*)part, N, a.slices, n, mean);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  a.mean = mean;
  if ((e = bn_sweep<BN_SQ>(a, s)) != hipSuccess) return e;
  const float d = (float)(1.0 - momentum);
  const float f = (float)((double)n / (double)(n > 1 ? n - 1 : 1));
  hipLaunchKernelGGL(bn_var_kernel, dim3(cols), dim3(256), 0, s, (const double*)part, N, a.slices, n, (const float*)mean, var, d, f,
                     bessel ? 1 : 0, mm, mv);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  BnApplyArgs b = {};
  b.z = z; b.ldz = ldz; b.n = n; b.N = N; b.mean = mean; b.var = var; b.gamma = gamma; b.beta = beta; b.act = act;
  b.out = y; b.ldo = ldy;
  hipLaunchKernelGGL(bn_apply_kernel<false>, dim3((unsigned)((n + kBnApplyRows - 1) / kBnApplyRows), (unsigned)((N + kBnApplyCols - 1) / kBnApplyCols)),
                     dim3(256), 0, s, b);
  return hipGetLastError();
}

hipError_t launch_bn_batch_backward(const float* gy, int64_t ldgy, const float* z, int64_t ldz, int64_t n, int N, const float* mean,
                                    const float* var, const float* gamma, const float* beta, int act, float* gz, int64_t ldgz,
                                    float* ggamma, float* gbeta, void* ws, hipStream_t s) {
  const BnLayout L = bn_layout(n, N);
  double* part = reinterpret_cast<double*>(static_cast<char*>(ws) + L.part);
  double* sums = reinterpret_cast<double*>(static_cast<char*>(ws) + L.sums);
  BnSweepArgs a = {};
  a.z = z; a.ldz = ldz; a.gy = gy; a.ldgy = ldgy; a.n = n; a.N = N; a.part = part;
  a.mean = mean; a.var = var; a.gamma = gamma; a.beta = beta; a.act = act;
  bn_slices(n, &a.rows_per_slice, &a.slices);
  hipError_t e;
  if ((e = bn_sweep<BN_GRAD>(a, s)) != hipSuccess) return e;
  hipLaunchKernelGGL(bn_grad_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, (const double*)part, N, a.slices, gbeta, ggamma,
                     sums);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  BnApplyArgs b = {};
  b.z = z; b.ldz = ldz; b.gy = gy; b.ldgy = ldgy; b.n = n; b.N = N; b.mean = mean; b.var = var; b.gamma = gamma; b.beta = beta;
  b.act = act; b.sums = sums; b.out = gz; b.ldo = ldgz;
  hipLaunchKernelGGL(bn_apply_kernel<true>, dim3((unsigned)((n + kBnApplyRows - 1) / kBnApplyRows), (unsigned)((N + kBnApplyCols - 1) / kBnApplyCols)),
                     dim3(256), 0, s, b);
  return hipGetLastError();
}

}  // namespace xv
