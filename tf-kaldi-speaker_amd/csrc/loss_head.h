// The margin head of the classifier losses, once for the forward (loss_rows_kernel, csrc/loss.hip) and the gradient
// (grad_label_kernel, csrc/loss_grad.hip): the target logit of the two must agree bit for bit (tests/test_gpu_loss_grad.py),
// so both evaluate it by the same calls.  Everything is double, from the stored rows; the caller rounds once.
#pragma once

#include "wave_reduce.h"
#include "xv_kernels.h"

namespace xv {

struct LossHead {
  int head;                 // XV_LOSS_*
  int m;                    // asoftmax: 1, 2 or 4
  double margin;            // additive margin
  double cos_m, sin_m;      // additive angular margin: cos m, sin m and cos(pi - m), from the host in double
  double cos_pi_m;
  double fa;                // 1 / (1 + lambda); 0 switches the margin off (asoftmax m = 1, softmax)
  double s;                 // grad_scale (the gradient only)
};

inline LossHead loss_head(int head, int m, double margin, double fa, double grad_scale) {
  LossHead hp = {};
  hp.head = head;
  hp.m = m;
  hp.margin = margin;
  hp.cos_m = cos(margin);
  hp.sin_m = sin(margin);
  hp.cos_pi_m = cos(3.14159265358979323846 - margin);
  hp.fa = (head == XV_LOSS_SOFTMAX || (head == XV_LOSS_ASOFTMAX && m == 1)) ? 0.0 : fa;
  hp.s = grad_scale;
  return hp;
}

// What one wave finds of row x [E] against the class row w [E]: dot = x . w, and with `norm` xn = ||x|| from the row scaled by
// the power of two of its largest element (exact, as row_prepare_kernel of csrc/score.hip; inf / nan rows are passed on),
// fn = max(xn, 1e-12) (tf.maximum(tf.norm(features, axis=1), eps)), craw = dot / fn and its clipped value c.
struct HeadRow {
  double dot, xn, fn, craw, c;
};

__device__ __forceinline__ HeadRow head_row(const float* __restrict__ xr, const float* __restrict__ wr, int E, int lane, bool norm) {
  HeadRow r = {};
  float mx = 0.f;
  double dot = 0.0;
  for (int c = lane; c < E; c += 64) {
    mx = fmaxf(mx, fabsf(xr[c]));
    dot = fma((double)xr[c], (double)wr[c], dot);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  r.dot = wave_sum_f64(dot);
  if (!norm) return r;
  if (mx > 0.f && mx <= 3.4028234e38f) {
    const int e = ilogbf(mx);                         // row * 2^-e has its largest element in [1, 2): exact scaling
    double ss = 0.0;
    for (int c = lane; c < E; c += 64) {
      const double v = (double)ldexpf(xr[c], -e);
      ss = fma(v, v, ss);
    }
    r.xn = ldexp(sqrt(wave_sum_f64(ss)), e);
  } else if (mx != 0.f) {
    r.xn = (double)mx;
  }
  r.fn = r.xn > 1e-12 ? r.xn : 1e-12;
  r.craw = r.dot / r.fn;
  const double lo = -1.0 + 1e-12, hi = 1.0 - 1e-12;
  r.c = r.craw < lo ? lo : (r.craw > hi ? hi : r.craw);
  return r;
}

// phi(c) of the head, and its derivative if `dphi` is given (1 where phi = c)
__device__ __forceinline__ double head_phi(const LossHead& hp, double c, double* dphi) {
  double phi = c, d = 1.0;
  if (hp.head == XV_LOSS_ASOFTMAX) {
    const double s0 = c > 0.0 ? 1.0 : (c < 0.0 ? -1.0 : 0.0);
    const double c2 = c * c;
    if (hp.m == 2) {
      phi = 2.0 * s0 * c2 - 1.0;                      // model/loss.py:159
      if (dphi) d = 4.0 * fabs(c);
    } else if (hp.m == 4) {                           // model/loss.py:161-166
      const double q = 2.0 * c2 - 1.0;
      const double s3 = (q > 0.0 ? 1.0 : (q < 0.0 ? -1.0 : 0.0)) * s0;
      const double s4 = 2.0 * s0 + s3 - 3.0;
      phi = s3 * (8.0 * c2 * c2 - 8.0 * c2 + 1.0) + s4;
      if (dphi) d = s3 * (32.0 * c2 * c - 16.0 * c);
    }
  } else if (hp.head == XV_LOSS_AMSOFTMAX) {
    phi = c - hp.margin;                              // model/loss.py:254
  } else {                                            // model/loss.py:343-352
    const double s2 = 1.0 - c * c;
    const double sn = sqrt(s2 > 1e-12 ? s2 : 1e-12);
    const double cpm = c * hp.cos_m - sn * hp.sin_m;
    const bool first = c > hp.cos_pi_m;
    phi = first ? cpm : -cpm - 2.0;
    if (dphi) {
      const double dsn = s2 > 1e-12 ? -c / sn : 0.0;
      const double dcpm = hp.cos_m - dsn * hp.sin_m;
      d = first ? dcpm : -dcpm;
    }
  }
  if (dphi) *dphi = d;
  return phi;
}

// the target logit behind the margin: fs z_label + fa ||x|| phi, fs = 1 - fa
__device__ __forceinline__ double head_target(const LossHead& hp, const HeadRow& r, double phi) {
  return (1.0 - hp.fa) * r.dot + hp.fa * (phi * r.fn);
}

}  // namespace xv
