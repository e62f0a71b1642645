// The lines every trained layer shares behind its product z: batch norm (inference mode), the activation, the activation's
// gradient and the three column sums of the backward pass.  csrc/seg_grad.hip (a dense layer, rows in panels) and
// csrc/tconv_grad.hip (a W-tap temporal convolution on packed utterances, rows in slices) compute z, gw and gx each in its own
// way and take everything between from here, so that forward and backward of both run the SAME instructions on the stored
// float z and the bounds below hold for both.  Contraction is ruled out by spelling every rounding.
//  * r_j = float(1 / sqrt(double(mv_j) + kBnEps)),  s_j = gamma_j * r_j,  d = z - mm_j,  h = fma(s_j, d, beta_j) (one
//    rounding); every step rounded to float32 on its own.  Without batch norm h = z.
//  * y = h (none), h > 0 ? h : 0 (ReLU), h > 0 ? h : float(0.2) * h (leaky ReLU).
//  * a = gy act'(h): gy (none), h > 0 ? gy : 0 (ReLU), h > 0 ? gy : float(0.2) * gy (leaky ReLU); h from the stored z by bn_h, so
//    the mask is the forward's.  gz = a * s_j (gz = a without batch norm).
//  * The column sums of the two mask kernels (seg_mask_kernel, tc_mask_kernel): lane l of the wave that owns column j adds the
//    rows i = l (mod 64) in ascending order to three doubles, a (gbeta), double(a) * (double(r_j) * (double(z) - double(mm_j)))
//    (ggamma) and gz (gbias); wave_sum_f64 (csrc/wave_reduce.h), a fixed xor butterfly over the 64 lanes, closes a sum before
//    its one rounding.  The two kernel bodies stay apart: which rows are live, gz^T and where the lane sums go differ, and so
//    does what the compiler makes of them.
//
// Error bound (u = 2^-24; checked per element in tests/test_gpu_seg_grad.py and tests/test_gpu_tconv.py, restated in
// ref_seg_grad.bounds).  |.| of the float64 oracle's values; Bz is the caller's bound of z_ij, n the rows summed; t = 2^-53
// (n + 64) covers the double sums of any order of n terms before their one rounding:
//   h_ij:      Bh = 1.01 |gamma_j r_j| Bz + 4 u |gamma_j r_j (z_ij - mm_j)| + u |h_ij|     (r, s and d round once each: 3 u, the
//              fourth u and the 1.01 cover the products of two errors; the fma rounds once).  Without batch norm Bh = Bz.
//   y_ij:      By = Bh + 2 u |y_ij|                     (the rounding of 0.2 and of the product; the sign of h is the oracle's
//              wherever |h| > Bh, which the test cases guarantee with a factor of 64, or where h = 0 exactly in both)
//   a_ij:      Ba = 2 u |a_ij|                          (leaky ReLU; 0 for ReLU and none, where a is gy or 0 exactly)
//   gz_ij:     Bg = |gamma_j r_j| Ba + 3.01 u |gz_ij|   (s carries 2 u, the product u); Bg = Ba without batch norm
//   gbeta_j:   sum_i Ba + (u + t) sum_i |a_ij|
//   ggamma_j:  sum_i (Ba |r_j (z_ij - mm_j)| + |a_ij r_j| Bz) + (2 u + t) sum_i |a_ij r_j (z_ij - mm_j)|   (r rounded, one rounding)
//   gbias_j:   sum_i Bg + (u + t) sum_i |gz_ij|
#pragma once

#include "wave_reduce.h"
#include "xv_kernels.h"

namespace xv {
namespace lines {

constexpr double kBnEps = 1e-3;               // tf.layers.batch_normalization default epsilon

__device__ __forceinline__ float bn_r(float mv) { return (float)(1.0 / sqrt((double)mv + kBnEps)); }
__device__ __forceinline__ float bn_h(float z, float s, float mm, float beta) { return fmaf(s, __fsub_rn(z, mm), beta); }
__device__ __forceinline__ float act_y(float h, int act) {
  if (act == XV_SEG_ACT_NONE) return h;
  return h > 0.f ? h : (act == XV_SEG_ACT_RELU ? 0.f : __fmul_rn(0.2f, h));
}
__device__ __forceinline__ float act_grad(float g, float h, int act) {
  return act == XV_SEG_ACT_NONE ? g : (h > 0.f ? g : (act == XV_SEG_ACT_RELU ? 0.f : __fmul_rn(0.2f, g)));
}

}  // namespace lines
}  // namespace xv
