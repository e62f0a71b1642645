// Forward and backward of one segment-level layer, dense + batch norm (inference mode) + activation, with the CURRENT weights:
// what training tdnn6 / tdnn7 (tdnn12 / tdnn13) together with the classifier head needs behind the frozen `pooling` node
// (egs/voxceleb/v1/nnet/lib/finetune.py:6-7, the noupdate_var_list route of model/trainer.py:309-320).  The rule is stated in
// include/xvec_hip.h (xv_seg_forward, xv_seg_backward) and restated in float64 numpy in tests/helpers/ref_seg_grad.py;
// torch.autograd of linear + eval-mode batch_norm + relu / leaky_relu(0.2) gives the same numbers (tests/test_seg_grad_host.py).
//
// The products run on the tile skeleton of csrc/nt_gemm.h, shared with csrc/loss_grad.hip: exact fp32 on
// v_mfma_f32_32x32x2_f32, 64 x 64 tiles, a K step of 32, zero-filled edges.  All stages are stream-ordered, no floating-point
// atomics anywhere:
//  * seg_gemm_kernel<EPI_FWD>: z = x . w^T + b, then h and y in the epilogue.  The chain of z_ij runs over k ascending from 0
//    (a function of K alone), the bias is added last: z = float(acc + b_j).
//  * The batch-norm line and the activation, in forward and backward the SAME device functions on the stored float z, are those
//    of csrc/layer_lines.h (bn_r, bn_h, act_y, act_grad), shared with csrc/tconv_grad.hip.
//  * backward, per PANEL of P rows (P a multiple of 64, at most 1024, as many as the workspace holds), in ascending row order:
//      - seg_mask_kernel, one workgroup per 32 columns: a = gy act'(h) by act_grad, gz = a * s_j, written as gz
//        [P, ldg] and gz^T [N, P]; the three double lane sums run over the rows of the WHOLE batch in ascending order and live
//        in the workspace between the panels; the butterfly over the 64 lanes comes after the last panel, rounded once;
//      - seg_gemm_kernel<EPI_OUT>: gx_panel = gz . (w^T)^T over a transposed copy of w, K = N;
//      - seg_gemm_kernel<EPI_ACC>: gw += gz^T . (x_panel^T)^T, K = P.  The accumulators START from what the earlier panels left
//        in gw, so the sum over the rows is ONE fmaf chain in ascending row index whatever P is (the scheme of
//        csrc/loss_grad.hip); the first panel starts from zero, not from what gw held.
// Every element of every output is a function of the inputs alone: one writer per element, a fixed order, no value read from
// memory this call did not write.  Row i of z, y and gx uses row i and the parameters only.
//
// Error bound (u = 2^-24; checked per element in tests/test_gpu_seg_grad.py, restated in ref_seg_grad.bounds).  |.| of the
// float64 oracle's values.  Bh, By, Ba, Bg and the bounds of gbeta, ggamma and gbias are derived in csrc/layer_lines.h from this Bz:
//   z_ij:      Bz = (K + 2) u (sum_k |x_ik w_jk| + |b_j|)                     (fmaf chain of length K, then the bias)
//   gw_jk:     sum_i Bg |x_ik| + (n + 32) u sum_i |gz_ij x_ik|               (fmaf chain of length n, padded to 32)
//   gx_ik:     sum_j Bg |w_jk| + (N + 2) u sum_j |gz_ij w_jk|                (fmaf chain of length N)
#include "layer_lines.h"
#include "nt_gemm.h"

namespace xv {

using ntg::gf32x16;
using ntg::up;

namespace {

constexpr int kSegMaxPanel = 1024;
constexpr int kSegPanelStep = 64;             // a panel is a whole number of 64-row chunks of seg_mask_kernel (and of K steps of gw)

enum { EPI_FWD = 0, EPI_OUT = 1, EPI_ACC = 2 };

struct SegGemmArgs {
  const float* A; int64_t lda; int M;         // [M, K]
  const float* B; int64_t ldb; int N;         // [N, K]
  int K;
  int nMt, nNt;
  // EPI_FWD
  const float *bias, *gamma, *beta, *mm, *mv;
  int act;
  float* z; int64_t ldz; float* y; int64_t ldy;
  // EPI_OUT, EPI_ACC
  float* out; int64_t ldo; int first;
};

template <bool VEC, int EPI>
__global__ __launch_bounds__(256, 2) void seg_gemm_kernel(SegGemmArgs p) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int mt = (int)(blockIdx.x % (unsigned)p.nMt), nt = (int)(blockIdx.x / (unsigned)p.nMt);
  const ntg::NtPos<64, 64> at(mt, nt);

  // EPI_ACC: the chain over the rows goes on from where the last panel left it
  gf32x16 acc[1][1];
  ntg::nt_acc_start(acc, at, EPI == EPI_ACC && !p.first, p.out, p.ldo, p.M, p.N);
  ntg::nt_mainloop<64, 64, VEC>(p.A, p.lda, p.M, p.B, p.ldb, p.N, p.K, at.m0, at.n0, acc, smem);

  const int gj = at.col(0);
  if (gj >= p.N) return;
  float bj = 0.f, s = 0.f, mm = 0.f, beta = 0.f;
  if (EPI == EPI_FWD) {
    bj = p.bias[gj];
    if (p.gamma) {
      s = __fmul_rn(p.gamma[gj], lines::bn_r(p.mv[gj]));
      mm = p.mm[gj];
      beta = p.beta[gj];
    }
  }
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int gi = at.row(0, e);
    if (gi >= p.M) continue;
    if (EPI == EPI_FWD) {
      const float z = __fadd_rn(acc[0][0][e], bj);
      const float h = p.gamma ? lines::bn_h(z, s, mm, beta) : z;
      p.z[(int64_t)gi * p.ldz + gj] = z;
      p.y[(int64_t)gi * p.ldy + gj] = lines::act_y(h, p.act);
    } else {
      p.out[(int64_t)gi * p.ldo + gj] = acc[0][0][e];
    }
  }
}

template <bool VEC, int EPI>
hipError_t launch_seg_gemm(const SegGemmArgs& a, hipStream_t s) {
  return ntg::nt_launch<seg_gemm_kernel<VEC, EPI>>(ntg::nt_smem_bytes<64, 64>(), (int64_t)a.nMt * a.nNt, a, s);
}

// ---------------------------------------------------------------------------------------------- mask, gz, gz^T, column sums
struct SegMaskArgs {
  const float* gy; int64_t ldgy;              // the panel's rows (pointers already offset by the panel's first row)
  const float* z; int64_t ldz;
  int rows, N;                                // rows of this panel; the panel's first row is a multiple of 64
  const float *gamma, *beta, *mm, *mv;        // all four or none
  int act;
  float* gz; int64_t ldg;                     // [P, ldg]
  float* gzt; int64_t ldgt;                   // [N, P]
  double* part;                               // [3][N][64] lane sums, kept between the panels
  int first, last;
  float *gbeta, *ggamma, *gbias;              // written after the last panel (gbeta, ggamma: with batch norm only)
};

constexpr int kMaskCols = 32;                 // columns per workgroup of seg_mask_kernel, 8 per wave

// the twin of tc_mask_kernel (csrc/tconv_grad.hip); csrc/layer_lines.h says what they share and why the two bodies stay apart
__global__ __launch_bounds__(256) void seg_mask_kernel(SegMaskArgs p) {
  constexpr int CW = kMaskCols / 4;
  __shared__ float ta[64][kMaskCols + 1], tz[64][kMaskCols + 1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j0 = (int)blockIdx.x * kMaskCols;
  const bool bn = p.gamma != nullptr;
  // phase 1 reads along the rows: a half wave takes 32 columns of one row
  const int c1 = lane & 31, rsub = 2 * wave + (lane >> 5);
  const int jc = j0 + c1;
  const bool jok = jc < p.N;
  float s1 = 1.f, mm1 = 0.f, beta1 = 0.f;
  if (bn && jok) {
    s1 = __fmul_rn(p.gamma[jc], lines::bn_r(p.mv[jc]));
    mm1 = p.mm[jc];
    beta1 = p.beta[jc];
  }
  // phase 2 sums along the columns: wave w owns the columns j0 + 8 w + c, lane = row of the 64-row chunk
  float s2[CW], r2[CW], mm2[CW];
  double sa[CW], sg[CW], sz[CW];
#pragma unroll
  for (int c = 0; c < CW; ++c) {
    const int j = j0 + CW * wave + c;
    s2[c] = 1.f; r2[c] = 0.f; mm2[c] = 0.f;
    sa[c] = sg[c] = sz[c] = 0.0;
    if (j < p.N) {
      if (bn) {
        r2[c] = lines::bn_r(p.mv[j]);
        s2[c] = __fmul_rn(p.gamma[j], r2[c]);
        mm2[c] = p.mm[j];
      }
      if (!p.first) {
        sa[c] = p.part[((int64_t)0 * p.N + j) * 64 + lane];
        sg[c] = p.part[((int64_t)1 * p.N + j) * 64 + lane];
        sz[c] = p.part[((int64_t)2 * p.N + j) * 64 + lane];
      }
    }
  }
  for (int i0 = 0; i0 < p.rows; i0 += 64) {
    for (int rl = rsub; rl < 64; rl += 8) {
      const int i = i0 + rl;
      float a = 0.f, z = 0.f;
      if (i < p.rows && jok) {
        z = p.z[(int64_t)i * p.ldz + jc];
        const float h = bn ? lines::bn_h(z, s1, mm1, beta1) : z;
        const float g = p.gy[(int64_t)i * p.ldgy + jc];
        a = lines::act_grad(g, h, p.act);
        p.gz[(int64_t)i * p.ldg + jc] = bn ? __fmul_rn(a, s1) : a;
      }
      ta[rl][c1] = a;
      tz[rl][c1] = z;
    }
    __syncthreads();
    const int i = i0 + lane;
    if (i < p.rows) {
#pragma unroll
      for (int c = 0; c < CW; ++c) {
        const int cl = CW * wave + c, j = j0 + cl;
        if (j < p.N) {
          const float a = ta[lane][cl];
          const float g = bn ? __fmul_rn(a, s2[c]) : a;          // the bits phase 1 wrote to gz
          p.gzt[(int64_t)j * p.ldgt + i] = g;
          sa[c] += (double)a;
          sg[c] += (double)a * ((double)r2[c] * ((double)tz[lane][cl] - (double)mm2[c]));
          sz[c] += (double)g;
        }
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int c = 0; c < CW; ++c) {
    const int j = j0 + CW * wave + c;
    if (j >= p.N) continue;                                       // uniform over the wave
    if (!p.last) {
      p.part[((int64_t)0 * p.N + j) * 64 + lane] = sa[c];
      p.part[((int64_t)1 * p.N + j) * 64 + lane] = sg[c];
      p.part[((int64_t)2 * p.N + j) * 64 + lane] = sz[c];
      continue;
    }
    const double a = wave_sum_f64(sa[c]), g = wave_sum_f64(sg[c]), z = wave_sum_f64(sz[c]);
    if (lane == 0) {
      if (bn) {
        p.gbeta[j] = (float)a;
        p.ggamma[j] = (float)g;
      }
      p.gbias[j] = (float)z;
    }
  }
}

struct SegLayout {
  int64_t ldg, ldt;                 // row of gz [P, ldg] and of w^T [K, ldt], floats
  int64_t part, wt, panel;          // byte offsets
  int64_t per_row;                  // bytes of the panel per row: gz, gz^T and x^T
};

SegLayout seg_layout(int K, int N) {
  SegLayout L;
  L.ldg = up(N, 4);
  L.ldt = up(N, 4);
  int64_t o = 0;
  L.part = o;  o += up((int64_t)3 * N * 64 * 8, 256);
  L.wt = o;    o += up((int64_t)K * L.ldt * 4, 256);
  L.panel = o;
  L.per_row = 4 * (L.ldg + (int64_t)N + K);
  return L;
}

int64_t seg_full_panel(int64_t n) { return n < kSegMaxPanel ? up(n, kSegPanelStep) : kSegMaxPanel; }

}  // namespace

int64_t seg_workspace_bytes(int64_t n, int K, int N, int least) {
  if (n <= 0 || K <= 0 || N <= 0) return 0;
  const SegLayout L = seg_layout(K, N);
  return L.panel + (least ? kSegPanelStep : seg_full_panel(n)) * L.per_row;
}

hipError_t launch_seg_forward(const float* x, int64_t ldx, int n, int K, const float* w, int64_t ldw, int N, const float* bias,
                              const float* gamma, const float* beta, const float* mm, const float* mv, int act, float* z, int64_t ldz,
                              float* y, int64_t ldy, hipStream_t s) {
  SegGemmArgs a = {};
  a.A = x; a.lda = ldx; a.M = n; a.B = w; a.ldb = ldw; a.N = N; a.K = K;
  a.nMt = (n + 63) / 64; a.nNt = (N + 63) / 64;
  a.bias = bias; a.gamma = gamma; a.beta = beta; a.mm = mm; a.mv = mv; a.act = act;
  a.z = z; a.ldz = ldz; a.y = y; a.ldy = ldy;
  const bool vec = aligned16(x) && aligned16(w) && ldx % 4 == 0 && ldw % 4 == 0;
  return vec ? launch_seg_gemm<true, EPI_FWD>(a, s) : launch_seg_gemm<false, EPI_FWD>(a, s);
}

hipError_t launch_seg_backward(const float* gy, int64_t ldgy, const float* x, int64_t ldx, const float* z, int64_t ldz, int n, int K,
                               const float* w, int64_t ldw, int N, const float* gamma, const float* beta, const float* mm,
                               const float* mv, int act, float* gx, int64_t ldgx, float* gw, float* gbias, float* ggamma,
                               float* gbeta, void* ws, int64_t ws_bytes, hipStream_t s) {
  const SegLayout L = seg_layout(K, N);
  char* wsb = static_cast<char*>(ws);
  double* part = reinterpret_cast<double*>(wsb + L.part);
  float* wt = reinterpret_cast<float*>(wsb + L.wt);
  hipError_t e;
  if (gx && (e = ntg::nt_transpose(w, ldw, (int64_t)N, (int64_t)K, wt, L.ldt, s)) != hipSuccess) return e;

  int64_t P = (ws_bytes - L.panel) / L.per_row / kSegPanelStep * kSegPanelStep;
  if (P > seg_full_panel(n)) P = seg_full_panel(n);
  float* G = reinterpret_cast<float*>(wsb + L.panel);
  float* GT = G + P * L.ldg;
  float* XT = GT + (int64_t)N * P;
  for (int64_t r0 = 0; r0 < n; r0 += P) {
    const int pn = (int)(n - r0 < P ? n - r0 : P);
    const float* xp = x + r0 * ldx;
    SegMaskArgs m = {};
    m.gy = gy + r0 * ldgy; m.ldgy = ldgy; m.z = z + r0 * ldz; m.ldz = ldz; m.rows = pn; m.N = N;
    m.gamma = gamma; m.beta = beta; m.mm = mm; m.mv = mv; m.act = act;
    m.gz = G; m.ldg = L.ldg; m.gzt = GT; m.ldgt = P; m.part = part;
    m.first = r0 == 0 ? 1 : 0; m.last = r0 + pn >= n ? 1 : 0;
    m.gbeta = gbeta; m.ggamma = ggamma; m.gbias = gbias;
    hipLaunchKernelGGL(seg_mask_kernel, dim3((unsigned)((N + kMaskCols - 1) / kMaskCols)), dim3(256), 0, s, m);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (gx) {
      SegGemmArgs b = {};
      b.A = G; b.lda = L.ldg; b.M = pn; b.B = wt; b.ldb = L.ldt; b.N = K; b.K = N;
      b.nMt = (pn + 63) / 64; b.nNt = (K + 63) / 64;
      b.out = gx + r0 * ldgx; b.ldo = ldgx;
      if ((e = launch_seg_gemm<true, EPI_OUT>(b, s)) != hipSuccess) return e;
    }
    if ((e = ntg::nt_transpose(xp, ldx, (int64_t)pn, (int64_t)K, XT, P, s)) != hipSuccess) return e;
    SegGemmArgs c = {};
    c.A = GT; c.lda = P; c.M = N; c.B = XT; c.ldb = P; c.N = K; c.K = pn;
    c.nMt = (N + 63) / 64; c.nNt = (K + 63) / 64;
    c.out = gw; c.ldo = ldw; c.first = r0 == 0 ? 1 : 0;
    if ((e = launch_seg_gemm<true, EPI_ACC>(c, s)) != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace xv
