// Classifier-head validation loss on the GPU: the softmax family of model/loss.py without the [n, C] logit matrix.
//
// The reference builds, per batch, logits = features . W (+ b), replaces the target logit by its margin form and hands
// the matrix to tf.losses.sparse_softmax_cross_entropy (mean over rows of logsumexp_c(z_ic) - z_i,label):
//   model/loss.py:9-48      softmax                              z = x W + b
//   model/loss.py:80-198    asoftmax                             z = x W^ (columns of W normalised, tf.nn.l2_normalize),
//   model/loss.py:201-286   additive_margin_softmax              cos t = z_label / max(||x||, 1e-12) clipped to +-(1 - 1e-12),
//   model/loss.py:289-384   additive_angular_margin_softmax      target = fs z_label + fa ||x|| phi(cos t), fa = 1 / (1 + lambda)
//   model/trainer.py:1097   insight's accuracy: argmax over the logits BEFORE the margin (endpoints["logits"])
// Here three kernels give, per row, loss, the target logit after the margin, the log-sum-exp and the top-1 class:
//
//  * loss_classes_kernel (once per checkpoint): kernel [E, C] -> class rows [C, E], normalised for the angular heads
//    (w / sqrt(max(sum w^2, 1e-12)), the sum in double: a column of any fp32 magnitude neither overflows nor flushes, a
//    zero column stays zero), left raw for softmax.  64 classes per workgroup through an LDS transpose: reads run along
//    C, writes along E.
//  * loss_rows_kernel: one wave per row.  ||x_i||, the target product x_i . w_label, the cosine, phi and the target logit in
//    double by the lines of csrc/loss_head.h (which the gradient shares), rounded once.  A margin multiplies an error of the
//    cosine by |phi'| (16 for m = 4, unbounded for the additive angle as |cos t| -> 1), so the one logit that goes through phi
//    is not taken from the fp32 tile.  A label outside [0, C) is never followed: the row gets NaN and a flag word is raised,
//    which xv_loss_classifier reads back BEFORE the tile kernel is launched and turns into XV_ERR_INVALID.
//  * loss_tile_kernel: z = x . rows^T, the exact-fp32 tile product of csrc/nt_gemm.h at 128 x 128 per workgroup, K = E taken
//    whole, tiles walked in the order of ntg::nt_tile.  The epilogue writes the tile (+ bias) over the operand buffers as
//    [128][144] floats and reduces every row with 16 lanes: lane s owns the columns s, s + 16, ... , s + 112.  Per (row, tile) it leaves four words in the workspace: the largest logit M with the target
//    swapped in (only the tile that owns column labels[i] sees the swap), S = sum_c exp(z_c - M), the largest logit before
//    the margin and its lowest column.  Columns >= C take no part.
//  * loss_finish_kernel: one wave per row; lane l merges the tiles l, l + 64, ... in ascending order, then a fixed xor
//    butterfly.  No floating-point atomics anywhere: repeats are bit-identical, and a row's result does not depend on
//    where the row sits in the batch (the order of the sums is a function of the column alone).
//
// Error bound (u = 2^-24; checked in tests/test_gpu_loss.py, the formula restated in tests/helpers/ref_loss.py):
//   logit:  |z - exact| <= B_i = (E + 8) u ||x_i|| max_c ||w_c|| (+ |b_c| u), the bound of csrc/score.hip: E u for the fmaf
//           chain of the MFMA, and of the 8 spare units: 1 the rounding of the normalised class rows, 1 the bias add, 2 + 2
//           the two subtractions z - M_tile and M_tile - M (each <= u (|z| + |M|), absorbed as a perturbation of the
//           logit), 1 loss = lse - target against |target|.
//   target: the margin form is evaluated in double from the stored rows: L_i B_i with L_i = max(1, fs + fa |phi'(cos t_i)|) (1 for
//           softmax, asoftmax m = 1 and the additive margin).
//   lse:    log-sum-exp is 1-Lipschitz in the max norm, so L_i B_i from the logits, plus k u (1 + |lse_i|) with
//             k(C) = 30 + ceil(ceil(C / 128) / 64) + 4 ceil(ln C):
//           expf 2 ulp = 4 u per term (twice: exp(z - M) in the tile, exp(M_tile - M) in the merge) and 1 u for their product;
//           the tile sum is 7 sequential adds per lane + 4 butterfly levels = 11 u; the merge (ceil(T / 64) - 1) + 6 adds;
//           logf 2 ulp = 4 u |log S| with 0 <= log S <= ln C (the largest term is exp(0)); lse = M + log S and
//           loss = lse - target one rounding each of at most u |lse| + u |loss|: 4 + 4 + 1 + 11 + 5 + ceil(T / 64) + 2 + 3 spare.
//   loss:   the sum of the target and the lse bounds.
#include "loss_head.h"
#include "nt_gemm.h"

namespace xv {

namespace {

constexpr int LBM = 128, LBN = 128;           // the tile of a workgroup
constexpr int LLDZ = 144;                     // row of the logit tile in LDS: 128 * 144 floats = the four operand tiles exactly
constexpr size_t kLossOperandBytes = ntg::nt_smem_bytes<LBM, LBN>();
constexpr size_t kLossRowBytes = (size_t)LBM * (sizeof(int32_t) + sizeof(float));     // labels and targets of the tile
constexpr int kLossHeaderBytes = 256;         // flag word in front of the partials
static_assert(LBM * LLDZ * sizeof(float) == kLossOperandBytes, "the logit tile reuses the operand buffers");

// ---------------------------------------------------------------------------------------------- class rows
// kernel [E, ldk >= C] -> rows [C, ldr >= E]; 64 classes per workgroup, lane = class while reading, lane = e while writing
__global__ __launch_bounds__(256) void loss_classes_kernel(const float* __restrict__ w, int64_t ldk, int E, int64_t C, int normalize,
                                                           float* __restrict__ rows, int64_t ldr) {
  __shared__ float tile[64][65];
  __shared__ double part[4][64];
  __shared__ double inv[64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t c0 = (int64_t)blockIdx.x * 64;
  const int64_t c = c0 + lane;
  if (normalize) {
    double ss = 0.0;
    if (c < C)
      for (int e = wave; e < E; e += 4) {
        const double v = (double)w[(int64_t)e * ldk + c];
        ss = fma(v, v, ss);
      }
    part[wave][lane] = ss;
    __syncthreads();
    if (wave == 0) {
      const double s = (part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane]);
      inv[lane] = 1.0 / sqrt(s > 1e-12 ? s : 1e-12);        // tf.nn.l2_normalize: x * rsqrt(max(sum x^2, 1e-12))
    }
    __syncthreads();
  }
  for (int e0 = 0; e0 < E; e0 += 64) {
    for (int el = wave; el < 64; el += 4) {
      const int e = e0 + el;
      float v = 0.f;
      if (e < E && c < C) {
        v = w[(int64_t)e * ldk + c];
        if (normalize) v = (float)((double)v * inv[lane]);
      }
      tile[el][lane] = v;
    }
    __syncthreads();
    for (int cl = wave; cl < 64; cl += 4)
      if (c0 + cl < C && e0 + lane < E) rows[(c0 + cl) * ldr + e0 + lane] = tile[lane][cl];
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------- rows
__global__ __launch_bounds__(256) void loss_rows_kernel(const float* __restrict__ x, int64_t ldx, int64_t n, int E,
                                                        const int32_t* __restrict__ labels, const float* __restrict__ rows,
                                                        int64_t ldr, int64_t C, const float* __restrict__ bias, LossHead hp,
                                                        float* __restrict__ target, int* __restrict__ flag) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= n) return;
  const int32_t lab = labels[r];
  if (lab < 0 || lab >= C) {            // never followed
    if (lane == 0) {
      target[r] = __builtin_nanf("");
      *flag = 1;
    }
    return;
  }
  const HeadRow row = head_row(x + r * ldx, rows + (int64_t)lab * ldr, E, lane, hp.fa != 0.0);     // csrc/loss_head.h
  double t = row.dot;
  if (hp.head == XV_LOSS_SOFTMAX)
    t = row.dot + (bias ? (double)bias[lab] : 0.0);
  else if (hp.fa != 0.0)
    t = head_target(hp, row, head_phi(hp, row.c, nullptr));
  if (lane == 0) target[r] = (float)t;
}

// ---------------------------------------------------------------------------------------------- tiles
struct LossArgs {
  const float* A; int64_t lda; int n;         // x [n, E]
  const float* B; int64_t ldb; int m;         // class rows [C, E]
  int d;
  const float* bias;                          // [C] or null
  const int32_t* labels;                      // [n]
  const float* target;                        // [n], from loss_rows_kernel
  float* pm; float* ps; float* rv; int32_t* ri;   // partials [n][nNt]
  int nMt, nNt;
};

template <bool VEC>
__global__ __launch_bounds__(256, 2) void loss_tile_kernel(LossArgs p) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* Z = smem;                     // [LBM][LLDZ], the epilogue's view of the operand tiles
  int32_t* lab = reinterpret_cast<int32_t*>(smem + LBM * LLDZ);           // [LBM]
  float* tgt = reinterpret_cast<float*>(lab + LBM);                       // [LBM]

  const int tid = threadIdx.x;
  const int64_t ntiles = (int64_t)p.nMt * p.nNt;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    int mt, nt;
    ntg::nt_tile(t, p.nMt, p.nNt, mt, nt);
    const ntg::NtPos<LBM, LBN> at(mt, nt);
    const int m0 = at.m0, n0 = at.n0;

    if (tid < LBM) {
      const bool ok = m0 + tid < p.n;
      lab[tid] = ok ? p.labels[m0 + tid] : -1;
      tgt[tid] = ok ? p.target[m0 + tid] : 0.f;
    }

    ntg::gf32x16 acc[2][2];            // acc[ai][bi]: 32 A rows x 32 B rows
    ntg::nt_acc_start(acc, at);
    // its first barrier publishes the labels and targets too
    ntg::nt_mainloop<LBM, LBN, VEC>(p.A, p.lda, p.n, p.B, p.ldb, p.m, p.d, m0, n0, acc, smem);

    // The operand tiles are dead (the loop ends on a barrier): the logits go over them.
#pragma unroll
    for (int bi = 0; bi < 2; ++bi) {
      const int jl = at.lcol(bi);
      const int gj = n0 + jl;
      const float b = (p.bias && gj < p.m) ? p.bias[gj] : 0.f;
#pragma unroll
      for (int ai = 0; ai < 2; ++ai)
#pragma unroll
        for (int e = 0; e < 16; ++e) Z[at.lrow(ai, e) * LLDZ + jl] = acc[ai][bi][e] + b;
    }
    __syncthreads();

    // 16 lanes per row, 16 rows at a time; lane s owns the columns s + 16 q.  Every lane runs every step (DPP); rows
    // beyond n hold zeros and are not stored.
    const int sub = tid & 15;
    const int ncols = min(LBN, p.m - n0);          // >= 1
#pragma unroll 1
    for (int rr = 0; rr < LBM; rr += 16) {
      const int il = rr + (tid >> 4);
      const int lcol = lab[il] - n0;               // the target's column in this tile, if 0 <= lcol < ncols
      const float tv = tgt[il];
      float z[8];
      float mu = -__builtin_inff(), mr = -__builtin_inff();
      int ir = 0x7fffffff;
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int col = sub + 16 * q;
        const float raw = Z[il * LLDZ + col];
        const bool in = col < ncols;
        z[q] = in ? (col == lcol ? tv : raw) : -__builtin_inff();
        mu = fmaxf(mu, z[q]);
        if (in && raw > mr) { mr = raw; ir = col; }
      }
      const float M = row16_max(mu);
      float s = 0.f;
#pragma unroll
      for (int q = 0; q < 8; ++q) s += expf(z[q] - M);       // exp(-inf) = 0 for the columns beyond C
      s = row16_sum(s);
      const float R = row16_max(mr);
      const int I = row16_min(mr == R ? ir : 0x7fffffff);
      const int gi = m0 + il;
      if (sub == 0 && gi < p.n) {
        const int64_t o = (int64_t)gi * p.nNt + nt;
        p.pm[o] = M;
        p.ps[o] = s;
        p.rv[o] = R;
        p.ri[o] = I == 0x7fffffff ? I : n0 + I;      // a tile of NaNs offers no column
      }
    }
    __syncthreads();       // the next tile's operands overwrite the logits
  }
}

// ---------------------------------------------------------------------------------------------- finish
__global__ __launch_bounds__(256) void loss_finish_kernel(const float* __restrict__ pm, const float* __restrict__ ps,
                                                          const float* __restrict__ rv, const int32_t* __restrict__ ri, int64_t n,
                                                          int T, const float* __restrict__ target, float* __restrict__ loss,
                                                          float* __restrict__ lse, int32_t* __restrict__ top1) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= n) return;
  const int64_t o = r * T;
  float M = -__builtin_inff(), R = -__builtin_inff();
  int I = 0x7fffffff;
  for (int t = lane; t < T; t += 64) {
    M = fmaxf(M, pm[o + t]);
    const float v = rv[o + t];
    if (v > R) { R = v; I = ri[o + t]; }         // ascending tiles: the first of equal maxima has the lowest column
  }
  float Rw = R;
#pragma unroll
  for (int k = 32; k > 0; k >>= 1) {
    M = fmaxf(M, __shfl_xor(M, k, 64));
    Rw = fmaxf(Rw, __shfl_xor(Rw, k, 64));
  }
  int Iw = R == Rw ? I : 0x7fffffff;
#pragma unroll
  for (int k = 32; k > 0; k >>= 1) Iw = min(Iw, __shfl_xor(Iw, k, 64));
  float s = 0.f;
  for (int t = lane; t < T; t += 64) s += ps[o + t] * expf(pm[o + t] - M);
#pragma unroll
  for (int k = 32; k > 0; k >>= 1) s += __shfl_xor(s, k, 64);
  if (lane == 0) {
    const float l = M + logf(s);
    lse[r] = l;
    loss[r] = l - target[r];
    top1[r] = Iw == 0x7fffffff ? 0 : Iw;        // a row of NaNs
  }
}

}  // namespace

hipError_t launch_loss_classes(const float* kernel, int64_t ldk, int E, int64_t C, int normalize, float* rows, int64_t ldr,
                               hipStream_t s) {
  if (C <= 0) return hipSuccess;
  hipLaunchKernelGGL(loss_classes_kernel, dim3((unsigned)((C + 63) / 64)), dim3(256), 0, s, kernel, ldk, E, C, normalize, rows, ldr);
  return hipGetLastError();
}

int64_t loss_workspace_bytes(int64_t n, int64_t C) {
  if (n <= 0 || C <= 0) return kLossHeaderBytes;
  return kLossHeaderBytes + 16 * n * ((C + LBN - 1) / LBN);
}

hipError_t launch_loss_rows(const float* x, int64_t ldx, int64_t n, int E, const int32_t* labels, const float* rows, int64_t ldr,
                            int64_t C, const float* bias, int head, int m, double margin, double fa, float* target, void* ws,
                            hipStream_t s) {
  const LossHead hp = loss_head(head, m, margin, fa, 0.0);
  int* flag = static_cast<int*>(ws);
  hipError_t e = hipMemsetAsync(flag, 0, sizeof(int), s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(loss_rows_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, x, ldx, n, E, labels, rows, ldr, C, bias, hp,
                     target, flag);
  return hipGetLastError();
}

hipError_t launch_loss_tiles(const float* x, int64_t ldx, int n, int E, const int32_t* labels, const float* rows, int64_t ldr, int C,
                             const float* bias, const float* target, float* loss, float* lse, int32_t* top1, void* ws,
                             hipStream_t s) {
  LossArgs p = {};
  p.A = x; p.lda = ldx; p.n = n; p.B = rows; p.ldb = ldr; p.m = C; p.d = E;
  p.bias = bias; p.labels = labels; p.target = target;
  p.nMt = (n + LBM - 1) / LBM;
  p.nNt = (C + LBN - 1) / LBN;
  const int64_t cells = (int64_t)n * p.nNt;
  float* base = reinterpret_cast<float*>(static_cast<char*>(ws) + kLossHeaderBytes);
  p.pm = base; p.ps = base + cells; p.rv = base + 2 * cells; p.ri = reinterpret_cast<int32_t*>(base + 3 * cells);
  int cus = 0;
  hipError_t e = compute_units(&cus);
  if (e != hipSuccess) return e;
  const int64_t ntiles = (int64_t)p.nMt * p.nNt;
  const int64_t grid = ntiles < (int64_t)cus * 16 ? ntiles : (int64_t)cus * 16;
  const size_t smem = kLossOperandBytes + kLossRowBytes;
  e = ntg::nt_vec(x, ldx, rows, ldr) ? ntg::nt_launch<loss_tile_kernel<true>>(smem, grid, p, s)
                                     : ntg::nt_launch<loss_tile_kernel<false>>(smem, grid, p, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(loss_finish_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, p.pm, p.ps, p.rv, p.ri, (int64_t)n, p.nNt,
                     target, loss, lse, top1);
  return hipGetLastError();
}

}  // namespace xv
