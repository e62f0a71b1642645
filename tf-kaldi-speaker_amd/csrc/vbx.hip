// VB-HMM resegmentation of clustered x-vectors (include/xvec_hip.h, xv_vbx): the Bayesian HMM over the x-vector sequence of a
// recording that current diarization recipes run after the first clustering ("VBx": Landini et al., "Bayesian HMM clustering
// of x-vector sequences", 2022).  Neither the reference tree nor Kaldi's x-vector recipe has the step: **parity unpinned**;
// the rule is stated in the header and restated in numpy by tests/helpers/ref_vbx.py.  Everything is double.
//
// Two kernels.  vbx_project_kernel is row-parallel over all rows of all recordings: four rows per workgroup staged in LDS,
// thread k owns row k of the affine and leaves rho_t = u_t sqrt(psi) and G_t in the workspace (u_tk is one chain of fused
// multiply-adds in column order, the offset added last; sum_k u_tk^2 one chain in k order).  vbx_kernel is one 256-thread
// workgroup per recording and runs all iterations; no workgroup waits for another, __syncthreads is the only synchronisation
// and there is no atomic of any kind.  An iteration:
//   A. N_s: four partial chains per speaker (t = q, q + 4, ..) added as (p0 + p1) + (p2 + p3).
//   B. gamma^T rho [S, r]: 4 x 4 register tiles, every entry one chain of fused multiply-adds in row order; alpha goes to LDS
//      (S r doubles, at most 128 KiB).  invL is not kept: inv_l() gives the same bits wherever it is evaluated.
//   C. per speaker (one thread, d order): c_s = sum_d (invL + alpha^2) psi_d and the speaker's share of the ELBO.
//   D. rho alpha^T [T, S]: 4 x 4 register tiles over d, logp to the workspace.
//      The two products are plain FMA loops, not v_mfma_f64_16x16x4_f64 tiles: at the sizes of a recording (T = 600, r = 128,
//      S = 12: under a million multiply-adds each) they are short beside E, which is serial in T.  Measured on one 8192-row
//      recording with 16 speakers, 40 iterations take 507 ms at r = 32 and 551 ms at r = 256 (profiles/vbx.md): eight times
//      the product work adds 9 %.  A fixed chain per entry also keeps the summation order trivially independent of the shape.
//   E. forward in wave 0 and backward in wave 1, side by side (both need only logp and pi), lane j = speaker j.  The
//      transition matrix is loop_prob I + (1 - loop_prob) 1 pi^T, so a step costs one cross-lane maximum, one exp, one
//      cross-lane sum and one log per lane: O(S) per frame.  The cross-lane operations are xor butterflies, which leave the
//      same bits in every lane.  The next frame's logp is loaded before the current frame's arithmetic.  logp, lfw, lbw
//      [T, S] and the per-frame logsumexp of lfw [T] live in the workspace.
//   F. gamma = exp(lfw + lbw - tll) by all threads; the sum of the pi update as four partial chains per speaker, as in A.
// Every byte of the workspace that is read has been written earlier in the same call.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <mutex>
#include <vector>

#include "wave_reduce.h"
#include "xv_kernels.h"

namespace xv {
namespace {

constexpr int kVbxThreads = 256;
constexpr int kVbxMaxSpk = 64;
constexpr int kVbxMaxDim = 256;
constexpr int kVbxMaxIn = 2048;
constexpr int kProjRows = 4;
constexpr double kLog2Pi = 1.8378770664093454835606594728112;

struct VbxGroup {      // one entry of the group table in the workspace
  int64_t row0;        // first row, relative to the first row of the call
  int64_t gam;         // double offset of the group in gamma (and in logp, lfw, lbw)
  int64_t pi;          // double offset of the group in pi
  int32_t t, s;
};

struct VbxArgs {
  const VbxGroup* groups;
  const double* rho;      // [N, r]
  const double* gconst;   // [N]
  double* logp;           // [sum T S]
  double* lfw;
  double* lbw;
  double* lse;            // [N]
  const double* psi;
  int r;
  double* gamma;
  double* pi;
  double fa, fb, loop, eps;
  int max_iters;
  int32_t* labels;        // [N]
  double* elbo;
  int32_t* iters;
};

struct VbxShared {
  double n[kVbxMaxSpk], cs[kVbxMaxSpk], es[kVbxMaxSpk], pi[kVbxMaxSpk];
  double part[4][kVbxMaxSpk];
  double psi[kVbxMaxDim];
  double tll, elbo_prev;
  int stop;
};

// Xor butterflies over the 64 lanes: every lane ends with the same bits.  The offsets are constants so that the compiler can
// pick the cheapest cross-lane move for each; a loop over only the lanes that S needs has a run-time offset and measured
// slower (profiles/vbx.md).
__device__ inline double wave_max(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}

// the maximum taken out of a log-domain sum; 0 when there is none to take (all terms -inf)
__device__ inline double finite_or_zero(double m) { return fabs(m) <= DBL_MAX ? m : 0.0; }

// 1 / (1 + (Fa/Fb N_s) psi_d): one fused multiply-add and one division, the same bits at every call site
__device__ inline double inv_l(double cn, double psi) { return 1.0 / fma(cn, psi, 1.0); }

__global__ __launch_bounds__(kVbxThreads) void vbx_project_kernel(const float* x, int64_t ldx, int64_t rows, int d, const double* affine,
                                                                   const double* psi, int r, double* rho, double* gconst) {
  __shared__ float xs[kProjRows][kVbxMaxIn];
  __shared__ double usq[kProjRows][kVbxMaxDim];
  const int tid = threadIdx.x;
  const int64_t r0 = (int64_t)blockIdx.x * kProjRows;
  for (int i = tid; i < kProjRows * d; i += kVbxThreads) {
    const int rr = i / d, c = i - rr * d;
    xs[rr][c] = r0 + rr < rows ? x[(r0 + rr) * ldx + c] : 0.f;
  }
  __syncthreads();
  if (tid < r) {
    const double* row = affine + (int64_t)tid * (d + 1);
    double acc[kProjRows];
#pragma unroll
    for (int k = 0; k < kProjRows; ++k) acc[k] = 0.0;
    for (int c = 0; c < d; ++c) {
      const double av = row[c];
#pragma unroll
      for (int k = 0; k < kProjRows; ++k) acc[k] = fma(av, (double)xs[k][c], acc[k]);
    }
    const double off = row[d], sq = sqrt(psi[tid]);
#pragma unroll
    for (int k = 0; k < kProjRows; ++k) {
      const double u = acc[k] + off;
      usq[k][tid] = u * u;
      if (r0 + k < rows) rho[(r0 + k) * r + tid] = u * sq;
    }
  }
  __syncthreads();
  if (tid < kProjRows && r0 + tid < rows) {
    double sum = 0.0;
    for (int k = 0; k < r; ++k) sum += usq[tid][k];
    gconst[r0 + tid] = -0.5 * (sum + (double)r * kLog2Pi);
  }
}

// wave 0: lfw [T, S], lse [T] and tll
__device__ void vbx_forward(const double* logp, double* lfw, double* lse, int T, int S, double loop, VbxShared& sh) {
  const int j = threadIdx.x & 63;
  const bool live = j < S;
  const double pi_j = sh.pi[j];
  const double w = (1.0 - loop) * pi_j;
  double cur = live ? logp[j] + log(pi_j) : -INFINITY;
  if (live) lfw[j] = cur;
  double nxt = (live && T > 1) ? logp[S + j] : 0.0;
  for (int t = 1; t < T; ++t) {
    const double lp = nxt;
    if (live && t + 1 < T) nxt = logp[(int64_t)(t + 1) * S + j];
    const double m0 = finite_or_zero(wave_max(cur));
    const double e = exp(cur - m0);
    const double tot = wave_sum_f64(e);
    if (j == 0) lse[t - 1] = m0 + log(tot);
    cur = live ? (lp + m0) + log(fma(loop, e, w * tot)) : -INFINITY;
    if (live) lfw[(int64_t)t * S + j] = cur;
  }
  const double m0 = finite_or_zero(wave_max(cur));
  const double tll = m0 + log(wave_sum_f64(exp(cur - m0)));
  if (j == 0) {
    lse[T - 1] = tll;
    sh.tll = tll;
  }
}

// wave 1: lbw [T, S]
__device__ void vbx_backward(const double* logp, double* lbw, int T, int S, double loop, VbxShared& sh) {
  const int j = threadIdx.x & 63;
  const bool live = j < S;
  const double pi_j = sh.pi[j];
  double cur = 0.0;
  if (live) lbw[(int64_t)(T - 1) * S + j] = 0.0;
  double nxt = live ? logp[(int64_t)(T - 1) * S + j] : 0.0;
  for (int t = T - 2; t >= 0; --t) {
    const double lp = nxt;      // logp of frame t + 1
    if (live) nxt = logp[(int64_t)t * S + j];
    const double v = live ? lp + cur : -INFINITY;
    const double m0 = finite_or_zero(wave_max(v));
    const double b = exp(v - m0);
    const double c = wave_sum_f64(pi_j * b);
    cur = m0 + log(fma(loop, b, (1.0 - loop) * c));
    if (live) lbw[(int64_t)t * S + j] = cur;
  }
}

__global__ __launch_bounds__(kVbxThreads) void vbx_kernel(VbxArgs a) {
  extern __shared__ double alpha[];      // [S, r]
  __shared__ VbxShared sh;
  const int tid = threadIdx.x;
  const VbxGroup grp = a.groups[blockIdx.x];
  const int T = grp.t, S = grp.s, r = a.r;
  if (T == 0) {
    if (tid == 0) a.iters[blockIdx.x] = 0;
    return;
  }
  const double* rho = a.rho + grp.row0 * r;
  const double* gconst = a.gconst + grp.row0;
  double* lse = a.lse + grp.row0;
  double* logp = a.logp + grp.gam;
  double* lfw = a.lfw + grp.gam;
  double* lbw = a.lbw + grp.gam;
  double* gamma = a.gamma + grp.gam;
  double* elbo = a.elbo + (int64_t)blockIdx.x * a.max_iters;
  const double ratio = a.fa / a.fb;
  const int ns = (S + 3) >> 2, nd = (r + 3) >> 2, nt = (T + 3) >> 2;
  const int lane = tid & 63, wave = tid >> 6;

  for (int i = tid; i < r; i += kVbxThreads) sh.psi[i] = a.psi[i];
  if (tid < kVbxMaxSpk) sh.pi[tid] = tid < S ? a.pi[grp.pi + tid] : 0.0;
  __syncthreads();

  int it = 0;
  for (;;) {
    // ---- A. N_s
    {
      double acc = 0.0;
      if (lane < S)
        for (int t = wave; t < T; t += 4) acc += gamma[(int64_t)t * S + lane];
      sh.part[wave][lane] = acc;
    }
    __syncthreads();
    if (tid < S) sh.n[tid] = (sh.part[0][tid] + sh.part[1][tid]) + (sh.part[2][tid] + sh.part[3][tid]);
    __syncthreads();

    // ---- B. alpha = Fa/Fb invL (gamma^T rho)
    for (int idx = tid; idx < ns * nd; idx += kVbxThreads) {
      const int si = idx / nd, s0 = si << 2, d0 = (idx - si * nd) << 2;
      int sc[4], dc[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        sc[i] = s0 + i < S ? s0 + i : S - 1;
        dc[i] = d0 + i < r ? d0 + i : r - 1;
      }
      double acc[4][4];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.0;
      for (int t = 0; t < T; ++t) {
        const double* gr = gamma + (int64_t)t * S;
        const double* rr = rho + (int64_t)t * r;
        double gv[4], rv[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          gv[i] = gr[sc[i]];
          rv[i] = rr[dc[i]];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[i][j] = fma(gv[i], rv[j], acc[i][j]);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (s0 + i < S && d0 + j < r)
            alpha[(s0 + i) * r + d0 + j] = ratio * inv_l(ratio * sh.n[s0 + i], sh.psi[d0 + j]) * acc[i][j];
    }
    __syncthreads();

    // ---- C. the per-speaker constant of logp and the speaker's share of the ELBO
    if (tid < S) {
      const double cn = ratio * sh.n[tid];
      double c = 0.0, e = 0.0;
      for (int d = 0; d < r; ++d) {
        const double il = inv_l(cn, sh.psi[d]), al = alpha[tid * r + d];
        const double a2 = al * al;
        c = fma(il + a2, sh.psi[d], c);
        e += ((log(il) - il) - a2) + 1.0;
      }
      sh.cs[tid] = c;
      sh.es[tid] = e;
    }
    __syncthreads();

    // ---- D. logp = Fa (rho alpha^T - c_s / 2 + G_t)
    for (int idx = tid; idx < nt * ns; idx += kVbxThreads) {
      const int ti = idx / ns, t0 = ti << 2, s0 = (idx - ti * ns) << 2;
      const double* rr[4];
      const double* ar[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        rr[i] = rho + (int64_t)(t0 + i < T ? t0 + i : T - 1) * r;
        ar[i] = alpha + (s0 + i < S ? s0 + i : S - 1) * r;
      }
      double acc[4][4];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.0;
      for (int d = 0; d < r; ++d) {
        double rv[4], av[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          rv[i] = rr[i][d];
          av[i] = ar[i][d];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[i][j] = fma(rv[i], av[j], acc[i][j]);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (t0 + i < T && s0 + j < S)
            logp[(int64_t)(t0 + i) * S + s0 + j] = a.fa * ((acc[i][j] - 0.5 * sh.cs[s0 + j]) + gconst[t0 + i]);
    }
    __syncthreads();

    // ---- E. forward and backward, one wave each
    if (wave == 0)
      vbx_forward(logp, lfw, lse, T, S, a.loop, sh);
    else if (wave == 1)
      vbx_backward(logp, lbw, T, S, a.loop, sh);
    __syncthreads();

    // ---- F. gamma, pi, ELBO
    const double tll = sh.tll;
    for (int64_t i = tid; i < (int64_t)T * S; i += kVbxThreads) gamma[i] = exp((lfw[i] + lbw[i]) - tll);
    {
      double acc = 0.0;
      if (lane < S)
        for (int t = 1 + wave; t < T; t += 4) {
          const int64_t i = (int64_t)t * S + lane;
          acc += exp(((lse[t - 1] + logp[i]) + lbw[i]) - tll);
        }
      sh.part[wave][lane] = acc;
    }
    __syncthreads();
    if (wave == 0) {
      double v = 0.0;
      if (lane < S) {
        const double sum = (sh.part[0][lane] + sh.part[1][lane]) + (sh.part[2][lane] + sh.part[3][lane]);
        v = exp((lfw[lane] + lbw[lane]) - tll) + ((1.0 - a.loop) * sh.pi[lane]) * sum;
      }
      const double total = wave_sum_f64(v);
      sh.pi[lane] = v / total;
      if (lane == 0) {
        double e = 0.0;
        for (int s = 0; s < S; ++s) e += sh.es[s];
        e = tll + 0.5 * a.fb * e;
        elbo[it] = e;
        sh.stop = (it > 0 && e - sh.elbo_prev < a.eps) || it == a.max_iters - 1;
        sh.elbo_prev = e;
      }
    }
    __syncthreads();
    ++it;
    if (sh.stop) break;
  }

  if (tid < S) a.pi[grp.pi + tid] = sh.pi[tid];
  for (int i = it + tid; i < a.max_iters; i += kVbxThreads) elbo[i] = NAN;
  if (tid == 0) a.iters[blockIdx.x] = it;
  for (int t = tid; t < T; t += kVbxThreads) {
    const double* gr = gamma + (int64_t)t * S;
    int best = 0;
    double bv = gr[0];
    for (int s = 1; s < S; ++s)
      if (gr[s] > bv) {
        bv = gr[s];
        best = s;
      }
    a.labels[grp.row0 + t] = best;
  }
}

int64_t vbx_table_bytes(int64_t num_groups) { return (32 * num_groups + 255) / 256 * 256; }

void free_table(void* p) { delete static_cast<std::vector<VbxGroup>*>(p); }

}  // namespace

int64_t vbx_workspace_bytes(int64_t num_groups, const int64_t* offsets, const int32_t* num_spk, int r) {
  const int64_t rows = offsets[num_groups] - offsets[0];
  int64_t cells = 0;
  for (int64_t g = 0; g < num_groups; ++g) cells += (offsets[g + 1] - offsets[g]) * num_spk[g];
  return vbx_table_bytes(num_groups) + (int64_t)sizeof(double) * (rows * (r + 2) + 3 * cells);
}

hipError_t launch_vbx(const float* x, int64_t ldx, const int64_t* offsets, const int32_t* num_spk, int64_t num_groups, int d,
                      const double* affine, const double* psi, int r, double* gamma, double* pi, double fa, double fb,
                      double loop_prob, int max_iters, double epsilon, int32_t* labels, double* elbo, int32_t* iters, void* ws,
                      hipStream_t stream) {
  static_assert(sizeof(VbxGroup) == 32, "the group table has 32 bytes per group");
  const int64_t rows = offsets[num_groups] - offsets[0];
  auto* table = new std::vector<VbxGroup>(num_groups);
  int64_t cells = 0, spk = 0;
  int max_spk = 1;
  for (int64_t g = 0; g < num_groups; ++g) {
    VbxGroup& e = (*table)[g];
    e.row0 = offsets[g] - offsets[0];
    e.gam = cells;
    e.pi = spk;
    e.t = (int32_t)(offsets[g + 1] - offsets[g]);
    e.s = num_spk[g];
    cells += (int64_t)e.t * e.s;
    spk += e.s;
    if (e.t > 0 && e.s > max_spk) max_spk = e.s;
  }
  double* base = reinterpret_cast<double*>(static_cast<char*>(ws) + vbx_table_bytes(num_groups));
  hipError_t e = hipMemcpyAsync(ws, table->data(), table->size() * sizeof(VbxGroup), hipMemcpyHostToDevice, stream);
  if (e == hipSuccess) {
    static std::mutex mu;            // per-device attribute; any thread may make the first launch on a device
    static size_t set_for[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    std::lock_guard<std::mutex> lock(mu);
    if (!set_for[dev & 63]) {
      e = hipFuncSetAttribute(reinterpret_cast<const void*>(vbx_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                              kVbxMaxSpk * kVbxMaxDim * (int)sizeof(double));
      if (e == hipSuccess) set_for[dev & 63] = 1;
    }
  }
  if (e == hipSuccess) {
    VbxArgs a;
    a.groups = static_cast<const VbxGroup*>(ws);
    double* rho = base;
    double* gconst = rho + rows * r;
    a.rho = rho;
    a.gconst = gconst;
    a.lse = gconst + rows;
    a.logp = a.lse + rows;
    a.lfw = a.logp + cells;
    a.lbw = a.lfw + cells;
    a.psi = psi;
    a.r = r;
    a.gamma = gamma;
    a.pi = pi;
    a.fa = fa;
    a.fb = fb;
    a.loop = loop_prob;
    a.eps = epsilon;
    a.max_iters = max_iters;
    a.labels = labels + offsets[0];
    a.elbo = elbo;
    a.iters = iters;
    if (rows > 0) {
      hipLaunchKernelGGL(vbx_project_kernel, dim3((unsigned)((rows + kProjRows - 1) / kProjRows)), dim3(kVbxThreads), 0, stream,
                         x + offsets[0] * ldx, ldx, rows, d, affine, psi, r, rho, gconst);
      e = hipGetLastError();
    }
    if (e == hipSuccess) {
      hipLaunchKernelGGL(vbx_kernel, dim3((unsigned)num_groups), dim3(kVbxThreads), (size_t)max_spk * r * sizeof(double), stream, a);
      e = hipGetLastError();
    }
  }
  // the copy may still be reading the table when this returns: it is freed in stream order, behind the copy
  if (hipLaunchHostFunc(stream, free_table, table) != hipSuccess) {
    (void)hipStreamSynchronize(stream);
    delete table;
  }
  return e;
}

}  // namespace xv
