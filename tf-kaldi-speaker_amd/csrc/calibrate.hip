// Score calibration and fusion on the GPU: the statistics of a prior-weighted logistic regression over a trial list, and the
// affine fusion it fits.
//
// The reference has no calibration step (its only fusion is misc/utils/average_score.py, an equal-weight mean of two score
// files; its recipes leave calibration to outside tools): **parity unpinned**.  include/xvec_hip.h states the rules and
// tests/helpers/ref_calibration.py restates them in float64 numpy.  K + 1 numbers are fitted to 10^7 .. 10^9 trials, so one
// Newton step is one pass over every trial with an exp, a log1p and a division in double per trial: that pass is here; the
// (K + 1) x (K + 1) solve and the line search are host numpy (tf-kaldi-speaker_amd/calibration.py).
//
// Arithmetic.  llr = ((w_1 s_1 + w_2 s_2) + ...) + b in double, ascending k, bias last, every product and every sum rounded
// on its own (`#pragma clang fp contract(off)` around them: hipcc contracts a * b + c into an fma by default, and its
// __dmul_rn / __dadd_rn are plain operators that do not prevent it), so that numpy written the same way gives the same
// bits; z = llr + tau.  With e = exp(-|z|) and q = 1 / (1 + e): sigma(|z|) = q, sigma(-|z|) = e q, softplus(x) =
// max(x, 0) + log1p(e) for x = z or -z: nothing overflows for either sign, and for |z| > 745 e is 0, softplus is its argument
// or 0 and the Hessian term is exactly 0.
//
//  * logreg_stats_kernel<K>: a workgroup of 256 threads owns kChunk = 16384 consecutive rows; thread t takes the rows
//    chunk * kChunk + 256 i + t, i = 0 .. 63, in that order.  Its 1 + (K + 1) + (K + 1)(K + 2) / 2 double sums (55 at K = 8)
//    and 19 counters stay in registers: K is a template parameter and every loop over them is unrolled (build() fails when
//    the compiler reports scratch for this kernel).  The 64 lanes of a wave are added by a shuffle tree (offsets 32, 16, .. 1),
//    the four waves in wave order by the threads 0 .. 54, and the workgroup's partial goes to the workspace,
//    [chunk][nd] doubles followed by [chunk][19] int64.
//  * logreg_reduce_kernel: one wave per output entry; lane l adds the partials l, l + 64, .. of the chunks in ascending order,
//    then the same shuffle tree.  No atomics of any kind: the partition and the order of every sum depend on (n, k) alone, so
//    the result is a pure function of the inputs, whatever the workspace beyond its least size and whatever lies behind row n.
//    n = 0 launches the second kernel alone, which writes zeros.
//  * score_fuse_kernel: out[i] = float(llr_i), one thread per row, one rounding to float.
// The padding columns k .. lds - 1 of a row are never read.
#include "xv_kernels.h"

namespace xv {

namespace {

constexpr int kChunk = 16384;          // rows per workgroup: fixed, so that the partition depends on n alone
constexpr int kThreads = 256;
constexpr int kCounts = 3 + 2 * XV_LOGREG_MAX_THRESHOLDS;      // n_tar, n_non, bad, miss[8], fa[8]

__host__ __device__ constexpr int logreg_nd(int k) { return 1 + (k + 1) + (k + 1) * (k + 2) / 2; }

struct LogregArgs {
  double theta[XV_LOGREG_MAX_SYSTEMS + 1];
  double tau, c_tar, c_non;
  double thr[XV_LOGREG_MAX_THRESHOLDS];        // unused ones are NaN: neither comparison below holds
};

// ((w_1 s_1 + w_2 s_2) + ...) + b without contraction; false when a score is not finite
template <int K>
__device__ __forceinline__ bool row_llr(const float* __restrict__ row, const double* theta, double (&a)[K], double& llr) {
#pragma clang fp contract(off)
  bool finite = true;
  double acc = 0.0;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const float s = row[k];
    finite = finite && (fabsf(s) <= 3.402823466e38f);       // false for inf and NaN
    a[k] = (double)s;
    const double p = theta[k] * a[k];
    acc = k == 0 ? p : acc + p;
  }
  llr = acc + theta[K];
  return finite;
}

template <int K>
__global__ __launch_bounds__(kThreads) void logreg_stats_kernel(const float* __restrict__ scores, int64_t lds, int64_t n,
                                                                const uint8_t* __restrict__ targets, LogregArgs p,
                                                                double* __restrict__ wsd, long long* __restrict__ wsc) {
  constexpr int ND = logreg_nd(K);
  __shared__ double red[kThreads / 64][ND];
  __shared__ int redc[kThreads / 64][kCounts];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t r0 = (int64_t)blockIdx.x * kChunk;
  const int64_t r1 = r0 + kChunk < n ? r0 + kChunk : n;

  double f = 0.0, g[K + 1], h[(K + 1) * (K + 2) / 2];
  int cnt[kCounts];
#pragma unroll
  for (int i = 0; i <= K; ++i) g[i] = 0.0;
#pragma unroll
  for (int i = 0; i < (K + 1) * (K + 2) / 2; ++i) h[i] = 0.0;
#pragma unroll
  for (int i = 0; i < kCounts; ++i) cnt[i] = 0;

  for (int64_t r = r0 + tid; r < r1; r += kThreads) {
    double a[K], llr;
    if (!row_llr<K>(scores + r * lds, p.theta, a, llr)) {
      ++cnt[2];
      continue;
    }
    const bool tar = targets[r] != 0;
    const int is_tar = tar ? 1 : 0, is_non = 1 - is_tar;
    cnt[0] += is_tar;
    cnt[1] += is_non;
    const double lf = (double)(float)llr;               // the thresholds are compared with the float32 llr, in double
#pragma unroll
    for (int j = 0; j < XV_LOGREG_MAX_THRESHOLDS; ++j) {         // bitwise, not &&: no branch per threshold
      cnt[3 + j] += is_tar & (int)(lf < p.thr[j]);
      cnt[3 + XV_LOGREG_MAX_THRESHOLDS + j] += is_non & (int)(lf >= p.thr[j]);
    }
    const double z = llr + p.tau;
    const double e = exp(-fabs(z));
    const double q = 1.0 / (1.0 + e);
    const double l1p = log1p(e);
    const double hi = q, lo = e * q;                    // sigma(|z|), sigma(-|z|)
    // target: softplus(-z), r = -sigma(-z); non-target: softplus(z), r = sigma(z)
    const double x = tar ? -z : z;
    const double sp = fmax(x, 0.0) + l1p;
    const double sg = x >= 0.0 ? hi : lo;               // sigma(x)
    const double c = tar ? p.c_tar : p.c_non;
    const double cr = tar ? -(c * sg) : c * sg;
    const double ch = c * hi * lo;
    f += c * sp;
#pragma unroll
    for (int i = 0; i < K; ++i) g[i] += cr * a[i];
    g[K] += cr;
    int t = 0;
#pragma unroll
    for (int i = 0; i < K; ++i) {
      const double hai = ch * a[i];
#pragma unroll
      for (int j = i; j < K; ++j) h[t++] += hai * a[j];
      h[t++] += hai;
    }
    h[t] += ch;
  }

  // wave tree, then the four waves in order
  auto wave_sum = [](double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
  };
  f = wave_sum(f);
  if (lane == 0) red[wave][0] = f;
#pragma unroll
  for (int i = 0; i <= K; ++i) {
    const double v = wave_sum(g[i]);
    if (lane == 0) red[wave][1 + i] = v;
  }
#pragma unroll
  for (int i = 0; i < (K + 1) * (K + 2) / 2; ++i) {
    const double v = wave_sum(h[i]);
    if (lane == 0) red[wave][2 + K + i] = v;
  }
#pragma unroll
  for (int i = 0; i < kCounts; ++i) {
    int v = cnt[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if (lane == 0) redc[wave][i] = v;
  }
  __syncthreads();
  if (tid < ND) wsd[(int64_t)blockIdx.x * ND + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
  if (tid >= 64 && tid < 64 + kCounts) {
    const int i = tid - 64;
    wsc[(int64_t)blockIdx.x * kCounts + i] = (long long)redc[0][i] + redc[1][i] + redc[2][i] + redc[3][i];
  }
}

// block e < nd: double entry e; block nd + i: counter i.  One wave per entry.
__global__ __launch_bounds__(64) void logreg_reduce_kernel(const double* __restrict__ wsd, const long long* __restrict__ wsc,
                                                           int64_t nchunks, int nd, double* __restrict__ stats,
                                                           long long* __restrict__ counts) {
  const int e = blockIdx.x, lane = threadIdx.x;
  if (e < nd) {
    double v = 0.0;
    for (int64_t c = lane; c < nchunks; c += 64) v += wsd[c * nd + e];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if (lane == 0) stats[e] = v;
  } else {
    const int i = e - nd;
    long long v = 0;
    for (int64_t c = lane; c < nchunks; c += 64) v += wsc[c * kCounts + i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if (lane == 0) counts[i] = v;
  }
}

__global__ __launch_bounds__(kThreads) void score_fuse_kernel(const float* __restrict__ scores, int64_t lds, int64_t n, int k,
                                                              LogregArgs p, float* __restrict__ out) {
#pragma clang fp contract(off)
  const int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (r >= n) return;
  const float* row = scores + r * lds;
  double acc = p.theta[0] * (double)row[0];
  for (int i = 1; i < k; ++i) {
    const double prod = p.theta[i] * (double)row[i];
    acc = acc + prod;
  }
  out[r] = (float)(acc + p.theta[k]);
}

int64_t logreg_chunks(int64_t n) { return n > 0 ? (n + kChunk - 1) / kChunk : 0; }

template <int K>
void launch_stats_k(const float* scores, int64_t lds, int64_t n, const uint8_t* targets, const LogregArgs& p, double* wsd,
                    long long* wsc, hipStream_t s) {
  hipLaunchKernelGGL((logreg_stats_kernel<K>), dim3((unsigned)logreg_chunks(n)), dim3(kThreads), 0, s, scores, lds, n, targets, p,
                     wsd, wsc);
}

}  // namespace

int64_t logreg_workspace_bytes(int64_t n, int k) {
  return logreg_chunks(n) * (int64_t)((logreg_nd(k) + kCounts) * 8);
}

hipError_t launch_logreg_stats(const float* scores, int64_t lds, int64_t n, int k, const uint8_t* targets, const double* theta,
                               double tau, double c_tar, double c_non, const double* thresholds, int num_thresholds, double* stats,
                               int64_t* counts, void* ws, hipStream_t s) {
  LogregArgs p;
  for (int i = 0; i <= XV_LOGREG_MAX_SYSTEMS; ++i) p.theta[i] = i <= k ? theta[i] : 0.0;
  p.tau = tau;
  p.c_tar = c_tar;
  p.c_non = c_non;
  for (int j = 0; j < XV_LOGREG_MAX_THRESHOLDS; ++j) p.thr[j] = j < num_thresholds ? thresholds[j] : __builtin_nan("");
  const int64_t nchunks = logreg_chunks(n);
  const int nd = logreg_nd(k);
  double* wsd = static_cast<double*>(ws);
  long long* wsc = reinterpret_cast<long long*>(wsd + nchunks * nd);
  if (nchunks > 0) {
    switch (k) {
      case 1: launch_stats_k<1>(scores, lds, n, targets, p, wsd, wsc, s); break;
      case 2: launch_stats_k<2>(scores, lds, n, targets, p, wsd, wsc, s); break;
      case 3: launch_stats_k<3>(scores, lds, n, targets, p, wsd, wsc, s); break;
      case 4: launch_stats_k<4>(scores, lds, n, targets, p, wsd, wsc, s); break;
      case 5: launch_stats_k<5>(scores, lds, n, targets, p, wsd, wsc, s); break;
      case 6: launch_stats_k<6>(scores, lds, n, targets, p, wsd, wsc, s); break;
      case 7: launch_stats_k<7>(scores, lds, n, targets, p, wsd, wsc, s); break;
      case 8: launch_stats_k<8>(scores, lds, n, targets, p, wsd, wsc, s); break;
      default: return hipErrorInvalidValue;
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(logreg_reduce_kernel, dim3((unsigned)(nd + kCounts)), dim3(64), 0, s, wsd, wsc, nchunks, nd, stats,
                     reinterpret_cast<long long*>(counts));
  return hipGetLastError();
}

hipError_t launch_score_fuse(const float* scores, int64_t lds, int64_t n, int k, const double* theta, float* out, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  LogregArgs p;
  for (int i = 0; i <= XV_LOGREG_MAX_SYSTEMS; ++i) p.theta[i] = i <= k ? theta[i] : 0.0;
  p.tau = p.c_tar = p.c_non = 0.0;
  for (int j = 0; j < XV_LOGREG_MAX_THRESHOLDS; ++j) p.thr[j] = 0.0;
  hipLaunchKernelGGL(score_fuse_kernel, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, scores, lds, n, k, p,
                     out);
  return hipGetLastError();
}

}  // namespace xv
