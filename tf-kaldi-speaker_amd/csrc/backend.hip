// Statistics for training the LDA + PLDA back-end on the GPU: the weighted second-moment (Gram) matrix of a set of x-vectors
// and per-class means, both in double.
//
// The reference trains its back-end with three Kaldi binaries (egs/voxceleb/v1/run.sh:384-400, egs/sre/v1/run.sh:399-411):
//   ivector-mean scp:xvector.scp mean.vec
//   ivector-compute-lda --total-covariance-factor=0.0 --dim=$lda_dim ... transform.mat
//   ivector-compute-plda ark:spk2utt ... plda
// The heavy part of all three is one operation, G = sum_r w_r (x_r - c)(x_r - c)^T over ~10^6 rows of dimension 512
// (~0.6 TFLOP), which Kaldi accumulates on one CPU thread in double.  That sum and the class means are computed here; the
// d x d linear algebra behind them is host numpy (tf-kaldi-speaker_amd/backend.py).  Kaldi is not part of the reference
// tree: **parity unpinned**, as csrc/post.hip and csrc/score.hip.
//
// Arithmetic.  y = (double)x - c is one rounding (none with c null); the A operand is y * w (one more rounding; w is applied
// to this operand only); products and sums are double, v_mfma_f64_16x16x4_f64.  A product of two fp32 values is exact in
// double, so without c and w the only error is the double accumulation.  The rate of v_mfma_f64_16x16x4_f64 on gfx950 is
// not in the programming guides this project follows and has not been measured here: the tile shape below was chosen for
// simplicity (one LDS read per MFMA), not tuned against a known issue rate.
//
//  * gram_partial_kernel: a workgroup owns one 64 x 64 tile of the upper triangle of G and one slice of rows.  It stages
//    16-row chunks of the centred (and, for A, weighted) panels in LDS as doubles, [k][64 + 16] (the pad puts the two k rows
//    a half-wave reads on disjoint banks), register-staged double buffering as score_tile_kernel; the loaders zero-fill the
//    edges of n and d themselves.  Each of the four waves holds a 32 x 32 block as 2 x 2 MFMA tiles.  Operand / result
//    lane layout of the f64 MFMA (pinned by the one-hot test of tests/test_gpu_backend.py, not assumed):
//      A: lane l holds A[i = l & 15][k = l >> 4];  B: lane l holds B[k = l >> 4][j = l & 15];
//      D: register e of lane l is D[i = (l >> 4) + 4 e][j = l & 15].
//    The partial tile goes to the caller's workspace, [slice][tile][64][64].
//  * gram_reduce_kernel: one thread per entry of a tile adds the partials of the slices in slice order and writes the
//    entry and its mirror (a diagonal tile: only its own upper triangle, so G == G^T bitwise although w sits on one operand).
//    No floating-point atomics anywhere: repeated calls are bit-identical.  n = 0 writes zeros.
//  * class_mean_kernel: one thread per (class, column), the index convention of speaker_mean_kernel (csrc/post.hip), the sum
//    in double in list order, divided by the count, c subtracted on request.  A class without rows gets zeros; a row index
//    outside [0, n) is never followed: the class gets NaN.
#include "xv_kernels.h"

namespace xv {

typedef double bf64x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int GT = 64;               // tile edge
constexpr int GKB = 16;              // rows per staged chunk
constexpr int GLD = GT + 16;         // padded LDS row (doubles)
constexpr int GTILE = GT * GT;
constexpr int kGramTargetGroups = 1024;   // workgroups aimed at; fixed, so that the slicing depends on (n, d) alone
constexpr int kGramMinSliceRows = 256;

struct GramPlan {
  int nT;                // tile rows
  int64_t ntiles;        // tiles of the upper triangle
  int64_t nslices, slice_rows;
};

GramPlan gram_plan(int64_t n, int d) {
  GramPlan p;
  p.nT = (d + GT - 1) / GT;
  p.ntiles = (int64_t)p.nT * (p.nT + 1) / 2;
  if (n <= 0) {
    p.nslices = 0;
    p.slice_rows = GKB;
    return p;
  }
  int64_t want = (kGramTargetGroups + p.ntiles - 1) / p.ntiles;
  const int64_t most = (n + kGramMinSliceRows - 1) / kGramMinSliceRows;
  if (want > most) want = most;
  if (want < 1) want = 1;
  p.slice_rows = ((n + want - 1) / want + GKB - 1) / GKB * GKB;
  p.nslices = (n + p.slice_rows - 1) / p.slice_rows;       // every slice has at least one row; at most kGramTargetGroups
  return p;
}

// linear index of the upper triangle, row by row -> (ti, tj), ti <= tj
__device__ __forceinline__ void tile_of(int t, int nT, int& ti, int& tj) {
  ti = 0;
  while (t >= nT - ti) {
    t -= nT - ti;
    ++ti;
  }
  tj = ti + t;
}

template <typename T>
__global__ __launch_bounds__(256) void gram_partial_kernel(const T* __restrict__ x, int64_t ldx, int64_t n, int d,
                                                           const double* __restrict__ c, const double* __restrict__ w,
                                                           int64_t slice_rows, int nT, double* __restrict__ ws) {
  __shared__ double As[2][GKB][GLD];
  __shared__ double Bs[2][GKB][GLD];
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  int ti, tj;
  tile_of((int)blockIdx.x, nT, ti, tj);

  // staging map: thread -> (row wave + 4 i of the chunk, column `col` of both panels)
  const int col = lane;
  const int ca = ti * GT + col, cb = tj * GT + col;
  const bool oka = ca < d, okb = cb < d;
  const double cca = c && oka ? c[ca] : 0.0, ccb = c && okb ? c[cb] : 0.0;
  const int64_t r0 = (int64_t)blockIdx.y * slice_rows;
  const int64_t r1 = r0 + slice_rows < n ? r0 + slice_rows : n;
  const int64_t nchunks = r1 > r0 ? (r1 - r0 + GKB - 1) / GKB : 0;

  double ra[GKB / 4], rb[GKB / 4];
  auto load_chunk = [&](int64_t ch) {
#pragma unroll
    for (int i = 0; i < GKB / 4; ++i) {
      const int64_t r = r0 + ch * GKB + wave + 4 * i;
      double a = 0.0, b = 0.0;
      if (r < r1) {
        const T* xr = x + r * ldx;
        if (oka) {
          a = (double)xr[ca] - cca;
          if (w) a *= w[r];
        }
        if (okb) b = (double)xr[cb] - ccb;
      }
      ra[i] = a;
      rb[i] = b;
    }
  };
  auto store_chunk = [&](int buf) {
#pragma unroll
    for (int i = 0; i < GKB / 4; ++i) {
      As[buf][wave + 4 * i][col] = ra[i];
      Bs[buf][wave + 4 * i][col] = rb[i];
    }
  };

  bf64x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[i][j][e] = 0.0;

  if (nchunks > 0) {
    load_chunk(0);
    store_chunk(0);
  }
  __syncthreads();
  const int l15 = lane & 15, lk = lane >> 4;
  for (int64_t ch = 0; ch < nchunks; ++ch) {
    const int cur = (int)(ch & 1);
    if (ch + 1 < nchunks) load_chunk(ch + 1);
#pragma unroll
    for (int kk = 0; kk < GKB / 4; ++kk) {
      const int k = kk * 4 + lk;
      const double a0 = As[cur][k][wm * 32 + l15], a1 = As[cur][k][wm * 32 + 16 + l15];
      const double b0 = Bs[cur][k][wn * 32 + l15], b1 = Bs[cur][k][wn * 32 + 16 + l15];
      acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
    }
    if (ch + 1 < nchunks) store_chunk(cur ^ 1);
    __syncthreads();
  }

  double* out = ws + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * GTILE;
#pragma unroll
  for (int ai = 0; ai < 2; ++ai)
#pragma unroll
    for (int bi = 0; bi < 2; ++bi)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int li = wm * 32 + ai * 16 + lk + 4 * e;
        const int lj = wn * 32 + bi * 16 + l15;
        out[li * GT + lj] = acc[ai][bi][e];
      }
}

__global__ __launch_bounds__(256) void gram_reduce_kernel(const double* __restrict__ ws, int64_t nslices, int64_t ntiles, int nT,
                                                          int d, double* __restrict__ g) {
  int ti, tj;
  tile_of((int)blockIdx.x, nT, ti, tj);
  const int idx = (int)blockIdx.y * 256 + threadIdx.x;
  const int li = idx >> 6, lj = idx & 63;
  const int gi = ti * GT + li, gj = tj * GT + lj;
  if (gi >= d || gj >= d) return;
  if (ti == tj && li > lj) return;             // written as the mirror of (lj, li)
  const double* p = ws + (int64_t)blockIdx.x * GTILE + idx;
  double s = 0.0;
  for (int64_t k = 0; k < nslices; ++k) s += p[k * ntiles * GTILE];
  g[(int64_t)gi * d + gj] = s;
  if (gi != gj) g[(int64_t)gj * d + gi] = s;
}

__global__ __launch_bounds__(256) void class_mean_kernel(const float* __restrict__ x, int64_t ldx, int64_t n, int dim,
                                                         const int32_t* __restrict__ off, const int32_t* __restrict__ index,
                                                         int64_t num_classes, const double* __restrict__ c,
                                                         double* __restrict__ out, int64_t ldo) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= num_classes * dim) return;
  const int64_t s = i / dim;
  const int col = (int)(i - s * dim);
  const int b = off[s], e = off[s + 1];
  double acc = 0.0;
  bool bad = false;
  for (int k = b; k < e; ++k) {
    const int64_t r = index[k];
    if (r < 0 || r >= n) {
      bad = true;
      continue;
    }
    acc += (double)x[r * ldx + col];
  }
  double m = e > b ? acc / (double)(e - b) : 0.0;
  if (e > b && c) m -= c[col];
  out[s * ldo + col] = bad ? __builtin_nan("") : m;
}

template <typename T>
hipError_t launch_gram(const T* x, int64_t ldx, int64_t n, int d, const double* c, const double* w, double* g, double* ws,
                       hipStream_t s) {
  const GramPlan p = gram_plan(n, d);
  if (p.nslices > 0) {
    hipLaunchKernelGGL((gram_partial_kernel<T>), dim3((unsigned)p.ntiles, (unsigned)p.nslices), dim3(256), 0, s, x, ldx, n, d, c,
                       w, p.slice_rows, p.nT, ws);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(gram_reduce_kernel, dim3((unsigned)p.ntiles, GTILE / 256), dim3(256), 0, s, ws, p.nslices, p.ntiles, p.nT, d,
                     g);
  return hipGetLastError();
}

}  // namespace

int64_t gram_f64_workspace_bytes(int64_t n, int d) {
  const GramPlan p = gram_plan(n, d);
  return p.nslices * p.ntiles * GTILE * (int64_t)sizeof(double);
}

hipError_t launch_gram_f64(const float* x, int64_t ldx, int64_t n, int d, const double* c, const double* w, double* g,
                           double* ws, hipStream_t s) {
  return launch_gram<float>(x, ldx, n, d, c, w, g, ws, s);
}

hipError_t launch_gram_f64_rows64(const double* x, int64_t ldx, int64_t n, int d, const double* c, const double* w, double* g,
                                  double* ws, hipStream_t s) {
  return launch_gram<double>(x, ldx, n, d, c, w, g, ws, s);
}

hipError_t launch_class_mean_f64(const float* x, int64_t ldx, int64_t n, int dim, const int32_t* off, const int32_t* index,
                                 int64_t num_classes, const double* c, double* out, int64_t ldo, hipStream_t s) {
  if (num_classes <= 0) return hipSuccess;
  const int64_t total = num_classes * dim;
  hipLaunchKernelGGL(class_mean_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, x, ldx, n, dim, off, index,
                     num_classes, c, out, ldo);
  return hipGetLastError();
}

}  // namespace xv
