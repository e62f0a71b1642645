// Loss AND gradients of the four classifier heads in one call: what training a new softmax layer on a frozen encoder needs
// (egs/voxceleb/v1/nnet/lib/finetune.py:6-7).  The rule is stated in include/xvec_hip.h (xv_loss_classifier_grad) and restated
// in float64 numpy in tests/helpers/ref_loss_grad.py; TensorFlow's autodiff of model/loss.py:9-48, 80-198, 201-286, 289-384
// followed by tf.losses.sparse_softmax_cross_entropy gives the same numbers (tests/test_loss_grad_host.py).
//
// Stages, all stream-ordered, no floating-point atomics anywhere:
//  * grad_normalize_kernel: raw class rows [C, ldc] -> normalised rows w^ in the workspace and q_c = sum_e w_ce^2 in double.
//    The sum runs in the order of loss_classes_kernel (csrc/loss.hip: four fma chains over e = k mod 4, then (p0 + p1) +
//    (p2 + p3)), so w^ has the bits xv_loss_prepare_classes writes.  Softmax skips this and uses the raw rows.
//  * the three forward kernels of csrc/loss.hip, unchanged, on those rows: loss, target logit, lse and top1 are the bits of
//    xv_loss_classifier.  The target goes to the workspace first and is copied out after the label check, so that a bad label
//    leaves every output untouched.
//  * grad_label_kernel, one wave per row: the label's entry G_il and the coefficient r_i / ||x_i|| in double from the stored
//    rows, by the lines loss_rows_kernel evaluates the target with (csrc/loss_head.h): the margin multiplies an error of the cosine by |phi'|, so this one entry
//    does not come from the fp32 tile.
//  * per PANEL of P rows (P a multiple of 32, at most 1024, as many as the workspace holds), in ascending row order:
//      - nt_gemm_kernel<EPI_G>: z = x . w^T again (the exact-fp32 tile product of csrc/nt_gemm.h), G_ic = s expf(z_ic - lse_i),
//        the entry at column l_i swapped for G_il by the tile that owns it; written as G [P, C] and G^T [C, P];
//      - grad_bias: one wave per class, lane l adds the rows i = l (mod 64) of the batch in ascending order to a double that
//        lives in the workspace between the panels; a fixed butterfly over the 64 lanes after the last panel;
//      - nt_gemm_kernel<EPI_X>: grad_x_panel = G . (w^T)^T, K = C over a transposed copy of the rows, 64 x 64 tiles (a
//        512 x 512 result is 64 tiles, not 16); the epilogue adds r_i x_i / ||x_i|| in double and rounds once;
//      - nt_gemm_kernel<EPI_ACC>: gw += G^T . (x_panel^T)^T, K = P.  The accumulators START from the value the earlier panels
//        left in grad_rows, so the sum over the rows is ONE fmaf chain in ascending row index whatever P is: P is a multiple
//        of the K step, every K step takes its rows in the same fixed order, and rows beyond n are zero-filled (adding
//        0 * 0 changes nothing but the sign of a zero, and it is added iff n is no multiple of 32, whatever P).  The first
//        panel starts from zero, not from what grad_rows held.
//  * grad_finish_kernel (angular heads), one wave per class: grad_rows_c = (gw_c - w^_c (w^_c . gw_c)) / sqrt(q_c) with w^ =
//    w / sqrt(q) and the product in double, or gw_c / 1e-6 where q_c <= 1e-12 (the floor of tf.nn.l2_normalize), in place.
// Every element of every output is a function of the inputs alone: a fixed order by row index (gw, grad_bias) or by class index
// (grad_x), one writer per element, no value read from memory this call did not write.  grad_x_i and the per-row outputs use
// row i and the class rows only, so they do not depend on the batch around row i.
//
// Error bound (u = 2^-24; checked per element in tests/test_gpu_loss_grad.py, restated in ref_loss_grad.bounds).  With B_i the
// logit bound and bl_i the lse bound of csrc/loss.hip, L_i = max(1, fs + fa |phi'|) with the phi' of the backward pass (0 where
// c_raw lies outside the clip range: there the target is fs z + const):
//   p_ic, c != l:   z and lse are off by at most B_i and bl_i, the subtraction z - lse rounds by u (|z| + |lse|), expf is 2 ulp
//                   = 4 u, s is rounded to float (u) and multiplied (u):  |dG_ic| <= e_i G_ic,
//                   e_i = 1.01 (B_i + bl_i + u (||x_i|| max||w|| + |lse_i|)) + 6 u      (1.01: exp(d) - 1 <= 1.01 d for d <= 0.01)
//   label entry:    p_il = exp(t_i - lse_i) in double with t_i off by L_i B_i: |dd_i| <= s p_il 1.01 (L_i B_i + bl_i).  The
//                   stored w^ moves the cosine by at most u, phi' by phi'' u and phi by |phi'| u (phi'' = 4, |96 c^2 - 16|, 0,
//                   sin m / sn^3 for asoftmax 2, 4, the additive margin and the additive angle):
//                   |dG_il| <= |dd_i| (fs + fa |phi'|) + |d_i| fa phi'' u + u |G_il|            (rounded once)
//                   |dr_i|  <= |dd_i| fa |phi - phi' c| + |d_i| fa (2 |phi'| + |c| phi'') u
//   grad_x_ie:      sum_c |dG_ic| |w^_ce|  +  (C + 2) u sum_c |G_ic w^_ce|   (fmaf chain of length C, the rounding of w^)
//                   + |dr_i| |x_ie| / ||x_i||  +  2 u |grad_x_ie|           (the r term and the last rounding)
//   gw_ce:          a_ce = sum_i |dG_ic| |x_ie| + (n + 32) u sum_i |G_ic x_ie|       (fmaf chain of length n, padded to 32)
//   grad_bias_c:    sum_i |dG_ic| + u |grad_bias_c|                                 (double sum, rounded once)
//   grad_rows_ce:   softmax: a_ce + u |grad_rows_ce|.  Angular: with D = sum_e |w^_ce| a_ce the error of w^_c . gw_c,
//                   (a_ce + |w^_ce| D) / sqrt(q_c) + 2 u |grad_rows_ce|; below the floor a_ce / 1e-6 + u |grad_rows_ce|.
#include "loss_head.h"
#include "nt_gemm.h"

namespace xv {

using ntg::gf32x16;
using ntg::gf32x4;
using ntg::up;

namespace {

constexpr int kMaxPanel = 1024;
constexpr int kPanelStep = 32;                // a panel is a whole number of K steps of the gw product

// ---------------------------------------------------------------------------------------------- normalised rows
// 16 classes per wave, 4 lanes per class: lane k of a class sums e = k, k + 4, ... (the order of loss_classes_kernel)
__global__ __launch_bounds__(256) void grad_normalize_kernel(const float* __restrict__ rows, int64_t ldc, int E, int64_t C,
                                                             float* __restrict__ what, int64_t ldh, double* __restrict__ q) {
  const int k = threadIdx.x & 3;
  const int64_t c = (int64_t)blockIdx.x * 64 + (threadIdx.x >> 2);
  const bool ok = c < C;
  const float* r = rows + (ok ? c : 0) * ldc;
  double ss = 0.0;
  if (ok)
    for (int e = k; e < E; e += 4) {
      const double v = (double)r[e];
      ss = fma(v, v, ss);
    }
  const double p1 = __shfl_xor(ss, 1, 64);              // k ^ 1
  const double a = (k & 1) ? p1 + ss : ss + p1;         // p0 + p1 (k < 2) or p2 + p3, the lower index first
  const double b = __shfl_xor(a, 2, 64);
  const double s = (k & 2) ? b + a : a + b;             // (p0 + p1) + (p2 + p3)
  if (!ok) return;
  const double inv = 1.0 / sqrt(s > 1e-12 ? s : 1e-12);
  for (int e = k; e < E; e += 4) what[c * ldh + e] = (float)((double)r[e] * inv);
  if (k == 0) q[c] = s;
}

// ---------------------------------------------------------------------------------------------- the label's entry
__global__ __launch_bounds__(256) void grad_label_kernel(const float* __restrict__ x, int64_t ldx, int64_t n, int E,
                                                         const int32_t* __restrict__ labels, const float* __restrict__ rows,
                                                         int64_t ldr, const float* __restrict__ bias, LossHead hp,
                                                         const float* __restrict__ lse, float* __restrict__ gl,
                                                         double* __restrict__ coef) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= n) return;
  const int32_t lab = labels[r];                  // checked by the forward before this launch
  const HeadRow row = head_row(x + r * ldx, rows + (int64_t)lab * ldr, E, lane, hp.fa != 0.0);     // csrc/loss_head.h
  const double l = (double)lse[r];
  double g, rc = 0.0;
  if (hp.fa == 0.0) {
    const double t = row.dot + ((hp.head == XV_LOSS_SOFTMAX && bias) ? (double)bias[lab] : 0.0);
    g = hp.s * (exp(t - l) - 1.0);
  } else {
    double dphi;
    const double phi = head_phi(hp, row.c, &dphi);
    dphi *= row.craw == row.c ? 1.0 : 0.0;        // tf.clip_by_value passes the gradient inside the clip range only
    const double d = hp.s * (exp(head_target(hp, row, phi) - l) - 1.0);
    g = d * ((1.0 - hp.fa) + hp.fa * dphi);
    const double rr = d * hp.fa * (phi - dphi * row.craw);
    rc = row.xn > 1e-12 ? rr / row.xn : 0.0;
  }
  if (lane == 0) {
    gl[r] = (float)g;
    coef[r] = rc;
  }
}

// ---------------------------------------------------------------------------------------------- C = A . B^T, exact fp32
enum { EPI_G = 0, EPI_X = 1, EPI_ACC = 2 };

struct NtArgs {
  const float* A; int64_t lda; int M;         // [M, K]
  const float* B; int64_t ldb; int N;         // [N, K]
  int K;
  int nMt, nNt;
  // EPI_G: rows are the panel's rows (row pointers already offset by the panel's first row)
  const float* bias; const int32_t* labels; const float* lse; const float* gl; float sf;
  float* G; int64_t ldg; float* GT; int64_t ldgt;
  // EPI_X: out = acc + coef_i x_ie
  const double* coef; const float* x; int64_t ldx;
  // EPI_X, EPI_ACC
  float* out; int64_t ldo; int first;
};

template <int BM, int BN, bool VEC, int EPI>
__global__ __launch_bounds__(256, 2) void nt_gemm_kernel(NtArgs p) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const ntg::NtPos<BM, BN> at((int)(blockIdx.x % (unsigned)p.nMt), (int)(blockIdx.x / (unsigned)p.nMt));

  // EPI_ACC: the chain over the rows goes on from where the last panel left it
  gf32x16 acc[at.AI][at.BI];
  ntg::nt_acc_start(acc, at, EPI == EPI_ACC && !p.first, p.out, p.ldo, p.M, p.N);
  ntg::nt_mainloop<BM, BN, VEC>(p.A, p.lda, p.M, p.B, p.ldb, p.N, p.K, at.m0, at.n0, acc, smem);

#pragma unroll
  for (int bi = 0; bi < at.BI; ++bi) {
    const int gj = at.col(bi);
    const bool jok = gj < p.N;
    float bj = 0.f;
    if (EPI == EPI_G) bj = (p.bias && jok) ? p.bias[gj] : 0.f;
#pragma unroll
    for (int ai = 0; ai < at.AI; ++ai)
#pragma unroll
      for (int e4 = 0; e4 < 4; ++e4) {
        const int gi0 = at.row(ai, 4 * e4);
        if (EPI == EPI_G) {
          gf32x4 g4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int gi = gi0 + e;
            if (gi < p.M && jok) {
              const float z = acc[ai][bi][4 * e4 + e] + bj;
              const float g = p.labels[gi] == gj ? p.gl[gi] : p.sf * expf(z - p.lse[gi]);
              g4[e] = g;
              p.G[(int64_t)gi * p.ldg + gj] = g;
            }
          }
          if (jok && gi0 < p.M) *reinterpret_cast<gf32x4*>(p.GT + (int64_t)gj * p.ldgt + gi0) = g4;   // gi0 + 3 < ldgt: both multiples of 4
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int gi = gi0 + e;
            if (gi < p.M && jok) {
              float v = acc[ai][bi][4 * e4 + e];
              if (EPI == EPI_X) v = (float)((double)v + p.coef[gi] * (double)p.x[(int64_t)gi * p.ldx + gj]);
              p.out[(int64_t)gi * p.ldo + gj] = v;
            }
          }
        }
      }
  }
}

// grad_bias: one wave per class.  Lane l owns the rows i = l (mod 64) of the WHOLE batch and adds them in ascending order to
// its double gb[c][l], which lives in the workspace between the panels (row0 is the panel's first row, a multiple of 32, so
// the lane of a row does not depend on the panel); the last panel adds the 64 lanes by a fixed xor butterfly and rounds once.
// The reads run along the rows of G^T: coalesced.
__global__ __launch_bounds__(256) void grad_bias_kernel(const float* __restrict__ GT, int64_t ldgt, int rows, int64_t row0, int64_t C,
                                                        int first, int last, double* __restrict__ gb, float* __restrict__ grad_bias) {
  const int lane = threadIdx.x & 63;
  const int64_t c = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= C) return;
  double a = first ? 0.0 : gb[c * 64 + lane];
  const float* g = GT + c * ldgt;
  for (int i = (int)((lane - row0) & 63); i < rows; i += 64) a += (double)g[i];
  if (!last) {
    gb[c * 64 + lane] = a;
    return;
  }
  a = wave_sum_f64(a);
  if (lane == 0) grad_bias[c] = (float)a;
}

// backward of tf.nn.l2_normalize(w, dim=0), one wave per class, in place over gw
__global__ __launch_bounds__(256) void grad_finish_kernel(const float* __restrict__ rows, int64_t ldc, int E, int64_t C,
                                                          const double* __restrict__ q, float* __restrict__ grad_rows) {
  const int lane = threadIdx.x & 63;
  const int64_t c = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= C) return;
  const float* w = rows + c * ldc;
  float* g = grad_rows + c * ldc;
  const double qc = q[c];
  if (!(qc > 1e-12)) {
    for (int e = lane; e < E; e += 64) g[e] = (float)((double)g[e] / 1e-6);
    return;
  }
  const double inv = 1.0 / sqrt(qc);
  double dot = 0.0;
  for (int e = lane; e < E; e += 64) dot = fma((double)w[e] * inv, (double)g[e], dot);
  dot = wave_sum_f64(dot);
  for (int e = lane; e < E; e += 64) g[e] = (float)(((double)g[e] - ((double)w[e] * inv) * dot) * inv);
}

template <int BM, int BN, bool VEC, int EPI>
hipError_t launch_nt(const NtArgs& a, hipStream_t s) {
  return ntg::nt_launch<nt_gemm_kernel<BM, BN, VEC, EPI>>(ntg::nt_smem_bytes<BM, BN>(), (int64_t)a.nMt * a.nNt, a, s);
}

struct GradLayout {
  int64_t ldh, ldt;                 // row of w^ [C, ldh] and of (w^)^T [E, ldt], floats
  int64_t fwd, what, q, wt, tgt, gl, coef, gb, panel;     // byte offsets
  int64_t per_row;                  // bytes of the panel per row: G, G^T and x^T
};

GradLayout grad_layout(int64_t n, int64_t C, int E) {
  GradLayout L;
  L.ldh = up(E, 4);
  L.ldt = up(C, 4);
  int64_t o = 0;
  L.fwd = o;   o += up(loss_workspace_bytes(n, C), 256);
  L.what = o;  o += up(C * L.ldh * 4, 256);
  L.q = o;     o += up(C * 8, 256);
  L.wt = o;    o += up((int64_t)E * L.ldt * 4, 256);
  L.tgt = o;   o += up(n * 4, 256);
  L.gl = o;    o += up(n * 4, 256);
  L.coef = o;  o += up(n * 8, 256);
  L.gb = o;    o += up(C * 64 * 8, 256);              // 64 lane sums per class
  L.panel = o;
  L.per_row = 4 * (L.ldt + C + E);
  return L;
}

int64_t full_panel(int64_t n) { return n < kMaxPanel ? up(n, kPanelStep) : kMaxPanel; }

}  // namespace

int64_t loss_grad_workspace_bytes(int64_t n, int64_t C, int E, int least) {
  if (n <= 0 || C <= 0 || E <= 0) return 0;
  const GradLayout L = grad_layout(n, C, E);
  return L.panel + (least ? kPanelStep : full_panel(n)) * L.per_row;
}

hipError_t launch_loss_grad_forward_rows(const float* x, int64_t ldx, int64_t n, int E, const int32_t* labels, const float* rows,
                                         int64_t ldc, int64_t C, const float* bias, int head, int m, double margin, double fa,
                                         void* ws, hipStream_t s) {
  const GradLayout L = grad_layout(n, C, E);
  char* w = static_cast<char*>(ws);
  const float* use = rows;
  int64_t ldu = ldc;
  if (head != XV_LOSS_SOFTMAX) {
    float* what = reinterpret_cast<float*>(w + L.what);
    hipLaunchKernelGGL(grad_normalize_kernel, dim3((unsigned)((C + 63) / 64)), dim3(256), 0, s, rows, ldc, E, C, what, L.ldh,
                       reinterpret_cast<double*>(w + L.q));
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    use = what;
    ldu = L.ldh;
  }
  return launch_loss_rows(x, ldx, n, E, labels, use, ldu, C, bias, head, m, margin, fa, reinterpret_cast<float*>(w + L.tgt),
                          w + L.fwd, s);
}

hipError_t launch_loss_grad_rest(const float* x, int64_t ldx, int n, int E, const int32_t* labels, const float* rows, int64_t ldc,
                                 int C, const float* bias, int head, int m, double margin, double fa, double grad_scale,
                                 float* loss, float* target, float* lse, int32_t* top1, float* grad_x, int64_t ldgx,
                                 float* grad_rows, float* grad_bias, void* ws, int64_t ws_bytes, hipStream_t s) {
  const GradLayout L = grad_layout(n, C, E);
  char* w = static_cast<char*>(ws);
  const bool angular = head != XV_LOSS_SOFTMAX;
  const float* use = angular ? reinterpret_cast<const float*>(w + L.what) : rows;
  const int64_t ldu = angular ? L.ldh : ldc;
  float* tgt = reinterpret_cast<float*>(w + L.tgt);
  float* gl = reinterpret_cast<float*>(w + L.gl);
  double* coef = reinterpret_cast<double*>(w + L.coef);
  double* gb = reinterpret_cast<double*>(w + L.gb);
  float* wt = reinterpret_cast<float*>(w + L.wt);

  hipError_t e = launch_loss_tiles(x, ldx, n, E, labels, use, ldu, C, bias, tgt, loss, lse, top1, w + L.fwd, s);
  if (e != hipSuccess) return e;
  e = hipMemcpyAsync(target, tgt, (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, s);
  if (e != hipSuccess) return e;

  const LossHead hp = loss_head(head, m, margin, fa, grad_scale);
  hipLaunchKernelGGL(grad_label_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, x, ldx, (int64_t)n, E, labels, use, ldu, bias,
                     hp, lse, gl, coef);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if (grad_x) {
    if ((e = ntg::nt_transpose(use, ldu, (int64_t)C, (int64_t)E, wt, L.ldt, s)) != hipSuccess) return e;
  }

  int64_t P = (ws_bytes - L.panel) / L.per_row / kPanelStep * kPanelStep;
  if (P > full_panel(n)) P = full_panel(n);
  float* G = reinterpret_cast<float*>(w + L.panel);
  float* GT = G + P * L.ldt;
  float* XT = GT + (int64_t)C * P;
  for (int64_t r0 = 0; r0 < n; r0 += P) {
    const int pn = (int)(n - r0 < P ? n - r0 : P);
    const float* xp = x + r0 * ldx;
    NtArgs a = {};
    a.A = xp; a.lda = ldx; a.M = pn; a.B = use; a.ldb = ldu; a.N = C; a.K = E;
    a.nMt = (pn + 127) / 128; a.nNt = (C + 127) / 128;
    a.bias = bias; a.labels = labels + r0; a.lse = lse + r0; a.gl = gl + r0; a.sf = (float)grad_scale;
    a.G = G; a.ldg = L.ldt; a.GT = GT; a.ldgt = P;
    e = ntg::nt_vec(xp, ldx, use, ldu) ? launch_nt<128, 128, true, EPI_G>(a, s) : launch_nt<128, 128, false, EPI_G>(a, s);
    if (e != hipSuccess) return e;
    if (grad_bias) {
      hipLaunchKernelGGL(grad_bias_kernel, dim3((unsigned)((C + 3) / 4)), dim3(256), 0, s, GT, P, pn, r0, (int64_t)C, r0 == 0 ? 1 : 0,
                         r0 + pn >= n ? 1 : 0, gb, grad_bias);
      if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if (grad_x) {
      NtArgs b = {};
      b.A = G; b.lda = L.ldt; b.M = pn; b.B = wt; b.ldb = L.ldt; b.N = E; b.K = C;
      b.nMt = (pn + 63) / 64; b.nNt = (E + 63) / 64;
      b.coef = coef + r0; b.x = xp; b.ldx = ldx; b.out = grad_x + r0 * ldgx; b.ldo = ldgx;
      e = launch_nt<64, 64, true, EPI_X>(b, s);
      if (e != hipSuccess) return e;
    }
    if ((e = ntg::nt_transpose(xp, ldx, (int64_t)pn, (int64_t)E, XT, P, s)) != hipSuccess) return e;
    NtArgs c = {};
    c.A = GT; c.lda = P; c.M = C; c.B = XT; c.ldb = P; c.N = E; c.K = pn;
    c.nMt = (C + 127) / 128; c.nNt = (E + 127) / 128;
    c.out = grad_rows; c.ldo = ldc; c.first = r0 == 0 ? 1 : 0;
    e = launch_nt<128, 128, true, EPI_ACC>(c, s);
    if (e != hipSuccess) return e;
  }
  if (angular) {
    hipLaunchKernelGGL(grad_finish_kernel, dim3((unsigned)((C + 3) / 4)), dim3(256), 0, s, rows, ldc, E, (int64_t)C,
                       reinterpret_cast<const double*>(w + L.q), grad_rows);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace xv
