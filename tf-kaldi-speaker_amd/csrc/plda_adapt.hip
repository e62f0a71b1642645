// Per-recording PCA adaptation of a PLDA model (include/xvec_hip.h, xv_plda_adapt): what Kaldi's ivector-plda-scoring-dense
// does in front of the score matrix of every recording (EstPca, ApplyPca, Plda::ApplyTransform).  Kaldi is absent from the
// reference tree: **parity unpinned**; the rule is stated in the header and restated in numpy by
// tests/helpers/ref_plda_adapt.py.  Everything is double.
//
// One 256-thread workgroup adapts one group from its rows to its affine; a workgroup takes the groups blockIdx.x,
// blockIdx.x + gridDim.x, ... and owns one slot of the workspace (four m x m double matrices, m = d rounded up to even), so
// the workspace bounds how many groups run at a time and nothing else: no workgroup waits for another, __syncthreads is the
// only synchronisation and there is no atomic of any kind.  Every sum is a chain of additions in index order owned by one
// thread (or a fixed tree over the 256 threads), so a group's outputs are a pure function of its rows, the model and
// target_energy.
//
//   1. mu: one thread per column adds the rows in row order.  C: 64 x 64 tiles of the upper triangle, 8 centred rows staged in
//      LDS at a time, a 4 x 4 block of entries per thread, every entry one chain of fused multiply-adds in row order, then one
//      division by n; the mirror is a copy, and inside a diagonal tile (i, j) and (j, i) are the same chain of the same
//      products.  With y = (double)x - mu that is the bound of xv_gram_f64, n 2^-53 sum_r |y_ri y_rj|, and one division.
//      (The f64 MFMA tiles of csrc/backend.hip spread one Gram matrix over the whole device; here the device is already
//      full of groups, one per workgroup, and plain FMAs keep the summation order trivially fixed.)
//   2. jacobi(): two-sided cyclic Jacobi.  The m indices are paired in round-robin order (index m - 1 stays, the others walk
//      round a circle): m / 2 disjoint pairs per step, m - 1 steps per sweep.  An odd d is padded with a zero row and column,
//      which no rotation touches.  A step has two phases split by barriers: (a) thread k computes the rotation of pair k from
//      the 2 x 2 diagonal block, Rutishauser's form t = sign(theta) / (|theta| + sqrt(theta^2 + 1)), theta = (a_qq - a_pp) /
//      (2 a_pq), and leaves (c, s, t) in LDS; (b) one thread per pair of pairs (k <= k') applies J_k^T . J_k' to the 2 x 2
//      block at their crossing and writes the block and its mirror (the matrix stays symmetric bit for bit; the row and the
//      column phase of the textbook step are the two halves of this one update), and one thread per (pair, column) rotates
//      the two rows of V^T.  A pair is rotated while |a_pq| > 2^-53 ||A||_F / m; a step in which no pair qualifies skips phase
//      (b); a sweep without a rotation ends the iteration.  Whether a pair rotated travels through one LDS word that every
//      thread reads behind the same barrier, so the trip counts are uniform, and the sweep counter is capped at 30: nothing can
//      spin.  The matrix lives in LDS while 8 m^2 bytes fit 128 KiB (d <= 128) and in the slot otherwise; V^T is in the slot.
//   3. the rest of the chain in the same workgroup: rank sort of the eigenvalues, the energy rule (thread 0, in descending
//      order), P with its signs, M = P A^-1, W' = M M^T, B' = M diag(psi) M^T, a right-looking Cholesky of W', L^-1 by one
//      forward substitution per column, K = L^-1 B' L^-T (upper triangle, mirrored), jacobi() on K, A' = U^T L^-1,
//      T = [A' P | -A' P m], the signs of T.  psi' is clamped at 0 from below (K is positive semi-definite up to rounding).
//
// A group falls back (dim = 0) when n < 2, when the trace is not > 0, when a Cholesky pivot is not > 0 or when an
// iteration meets its sweep cap; eigval is written whenever n >= 2.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>
#include <vector>

#include "xv_kernels.h"

namespace xv {
namespace {

constexpr int kAdaptThreads = 256;
constexpr int kAdaptMaxDim = 256;
constexpr int kAdaptLdsDim = 128;        // the Jacobi matrix of m <= 128 lives in LDS: 8 m^2 <= 128 KiB of the CU's 160
constexpr int kAdaptSweepCap = 30;
constexpr int kAdaptMaxSlots = 1024;     // workgroups of one launch
constexpr int kPanelRows = 8;

struct AdaptArgs {
  const float* x;
  int64_t ldx;
  const int64_t* offsets;     // [G + 1], in the workspace
  int32_t* sweeps;            // [G, 2], in the workspace: sweeps of the two iterations (-1: cap met, 0: not run)
  int64_t num_groups;
  int d;
  const double* mean;
  const double* ainv;
  const double* psi;
  double target_energy;
  int32_t* dim;
  double* eigval;
  double* pca;
  double* affine;
  double* psi_out;
  double* slots;
  int64_t slot_doubles;
  int use_lds;
};

struct AdaptShared {
  double c[kAdaptMaxDim / 2], s[kAdaptMaxDim / 2], t[kAdaptMaxDim / 2];
  int p[kAdaptMaxDim / 2], q[kAdaptMaxDim / 2];
  double red[kAdaptThreads];
  double lam[kAdaptMaxDim];
  double vec[kAdaptMaxDim];
  double pan[2][kPanelRows][64];
  int perm[kAdaptMaxDim];
  int rot[2];
  int r;
};

// sum over the workgroup in a fixed tree; every thread gets the result
__device__ double block_sum(double v, AdaptShared& sh) {
  const int tid = threadIdx.x;
  __syncthreads();
  sh.red[tid] = v;
  __syncthreads();
  for (int o = kAdaptThreads / 2; o > 0; o >>= 1) {
    if (tid < o) sh.red[tid] += sh.red[tid + o];
    __syncthreads();
  }
  const double out = sh.red[0];
  __syncthreads();
  return out;
}

// Eigen-iteration of the symmetric a [m, lda] (m even), both triangles kept; vt [m, ldv] starts as the caller left it (the
// identity) and ends with the eigenvectors as rows, the eigenvalues on the diagonal of a.  Returns the number of sweeps that
// rotated something, or -1 when the cap was met.  The return value is the same in every thread.
__device__ int jacobi(double* a, int lda, double* vt, int ldv, int m, AdaptShared& sh) {
  const int tid = threadIdx.x;
  const int h = m >> 1;
  double acc = 0.0;
  for (int i = tid; i < m * m; i += kAdaptThreads) {
    const double v = a[(i / m) * lda + (i % m)];
    acc += v * v;
  }
  if (tid == 0) sh.rot[0] = 0;
  const double thr = sqrt(block_sum(acc, sh)) * 0x1p-53 / (double)m;
  const int fold_rows = (h + 1) >> 1, fold_w = h + 1;
  int gstep = 0;
  for (int sweep = 0; sweep < kAdaptSweepCap; ++sweep) {
    int any = 0;
    for (int step = 0; step < m - 1; ++step, ++gstep) {
      const int slot = gstep & 1;
      if (tid < h) {
        int i0, i1;
        if (tid == 0) {
          i0 = m - 1;
          i1 = step;
        } else {
          i0 = (step + tid) % (m - 1);
          i1 = (step - tid + (m - 1)) % (m - 1);
        }
        const int p = i0 < i1 ? i0 : i1, q = i0 < i1 ? i1 : i0;
        const double apq = a[p * lda + q];
        double c = 1.0, s = 0.0, t = 0.0;
        if (fabs(apq) > thr) {
          const double theta = (a[q * lda + q] - a[p * lda + p]) / (2.0 * apq);
          t = copysign(1.0, theta) / (fabs(theta) + sqrt(theta * theta + 1.0));
          if (t != 0.0) {
            c = 1.0 / sqrt(t * t + 1.0);
            s = t * c;
            sh.rot[slot] = 1;
          }
        }
        sh.c[tid] = c;
        sh.s[tid] = s;
        sh.t[tid] = t;
        sh.p[tid] = p;
        sh.q[tid] = q;
      }
      if (tid == 0) sh.rot[slot ^ 1] = 0;
      __syncthreads();
      const int rot = sh.rot[slot];
      any |= rot;
      if (rot) {
        // pairs of pairs k <= k2: the rows k and h - 1 - k of that triangle side by side are h + 1 long
        for (int idx = tid; idx < fold_rows * fold_w; idx += kAdaptThreads) {
          const int fa = idx / fold_w, fb = idx - fa * fold_w;
          int k, k2;
          if (fb < h - fa) {
            k = fa;
            k2 = fa + fb;
          } else {
            k = h - 1 - fa;
            if (k == fa) continue;
            k2 = k + (fb - (h - fa));
          }
          const double c1 = sh.c[k], s1 = sh.s[k], c2 = sh.c[k2], s2 = sh.s[k2];
          if (s1 == 0.0 && s2 == 0.0) continue;
          const int p1 = sh.p[k], q1 = sh.q[k];
          if (k == k2) {
            const double tt = sh.t[k] * a[p1 * lda + q1];
            a[p1 * lda + p1] -= tt;
            a[q1 * lda + q1] += tt;
            a[p1 * lda + q1] = 0.0;
            a[q1 * lda + p1] = 0.0;
            continue;
          }
          const int p2 = sh.p[k2], q2 = sh.q[k2];
          const double b11 = a[p1 * lda + p2], b12 = a[p1 * lda + q2], b21 = a[q1 * lda + p2], b22 = a[q1 * lda + q2];
          const double r11 = c1 * b11 - s1 * b21, r12 = c1 * b12 - s1 * b22;
          const double r21 = s1 * b11 + c1 * b21, r22 = s1 * b12 + c1 * b22;
          const double n11 = c2 * r11 - s2 * r12, n12 = s2 * r11 + c2 * r12;
          const double n21 = c2 * r21 - s2 * r22, n22 = s2 * r21 + c2 * r22;
          a[p1 * lda + p2] = n11;
          a[p2 * lda + p1] = n11;
          a[p1 * lda + q2] = n12;
          a[q2 * lda + p1] = n12;
          a[q1 * lda + p2] = n21;
          a[p2 * lda + q1] = n21;
          a[q1 * lda + q2] = n22;
          a[q2 * lda + q1] = n22;
        }
        for (int idx = tid; idx < h * m; idx += kAdaptThreads) {
          const int k = idx / m, col = idx - k * m;
          const double s = sh.s[k];
          if (s == 0.0) continue;
          const double c = sh.c[k];
          double* vp = vt + sh.p[k] * ldv + col;
          double* vq = vt + sh.q[k] * ldv + col;
          const double x = *vp, y = *vq;
          *vp = c * x - s * y;
          *vq = s * x + c * y;
        }
      }
      __syncthreads();
    }
    if (!any) return sweep;
  }
  return -1;
}

// sh.lam[0 .. cnt) -> sh.perm[rank] = index, descending, equal values by index.  A NaN compares false with everything, so every
// NaN entry gets rank 0 and the ranks behind keep the identity written first: no order, but every perm[] stays a valid index
// (a NaN spectrum has a NaN trace and falls back before perm is used)
__device__ void rank_sort(int cnt, AdaptShared& sh) {
  const int tid = threadIdx.x;
  if (tid < kAdaptMaxDim) sh.perm[tid] = tid;
  __syncthreads();
  if (tid < cnt) {
    const double v = sh.lam[tid];
    int rank = 0;
    for (int j = 0; j < cnt; ++j) {
      const double w = sh.lam[j];
      rank += (w > v) || (w == v && j < tid);
    }
    sh.perm[rank] = tid;
  }
  __syncthreads();
}

// +1 or -1 so that the entry of largest magnitude of row[0 .. cnt), the lowest column among equals, becomes positive
__device__ double row_sign(const double* row, int cnt) {
  double best = -1.0, sign = 1.0;
  for (int j = 0; j < cnt; ++j) {
    const double v = row[j];
    if (fabs(v) > best) {
      best = fabs(v);
      sign = v < 0.0 ? -1.0 : 1.0;
    }
  }
  return sign;
}

__global__ __launch_bounds__(kAdaptThreads) void plda_adapt_kernel(AdaptArgs g) {
  extern __shared__ double lds_matrix[];
  __shared__ AdaptShared sh;
  const int tid = threadIdx.x;
  const int d = g.d, m = d + (d & 1);
  const int64_t mm = (int64_t)m * m;
  double* slot = g.slots + (int64_t)blockIdx.x * g.slot_doubles;
  double* r0 = g.use_lds ? lds_matrix : slot;      // the four m x m regions of this workgroup
  double* r1 = slot + mm;
  double* r2 = slot + 2 * mm;
  double* r3 = slot + 3 * mm;

  for (int64_t grp = blockIdx.x; grp < g.num_groups; grp += gridDim.x) {
    __syncthreads();
    const int64_t row0 = g.offsets[grp];
    const int64_t n = g.offsets[grp + 1] - row0;
    int32_t* sweeps = g.sweeps + 2 * grp;
    if (n < 2) {
      if (tid == 0) {
        g.dim[grp] = 0;
        sweeps[0] = 0;
        sweeps[1] = 0;
      }
      continue;
    }
    const float* x = g.x + row0 * g.ldx;

    // ---- 1. mean and covariance
    if (tid < d) {
      double sum = 0.0;
      for (int64_t r = 0; r < n; ++r) sum += (double)x[r * g.ldx + tid];
      sh.vec[tid] = sum / (double)n;
    }
    __syncthreads();
    const int nt = (d + 63) >> 6;
    const int tx = tid & 15, ty = tid >> 4;
    for (int ti = 0; ti < nt; ++ti)
      for (int tj = ti; tj < nt; ++tj) {
        double acc[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[i][j] = 0.0;
        for (int64_t c0 = 0; c0 < n; c0 += kPanelRows) {
#pragma unroll
          for (int i = 0; i < 2 * kPanelRows * 64 / kAdaptThreads; ++i) {
            const int e = tid + kAdaptThreads * i;
            const int panel = e / (kPanelRows * 64), rr = (e >> 6) % kPanelRows, cc = e & 63;
            const int col = (panel ? tj : ti) * 64 + cc;
            const int64_t r = c0 + rr;
            sh.pan[panel][rr][cc] = (r < n && col < d) ? (double)x[r * g.ldx + col] - sh.vec[col] : 0.0;
          }
          __syncthreads();
#pragma unroll
          for (int rr = 0; rr < kPanelRows; ++rr) {
            double av[4], bv[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              av[i] = sh.pan[0][rr][ty * 4 + i];
              bv[i] = sh.pan[1][rr][tx * 4 + i];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
              for (int j = 0; j < 4; ++j) acc[i][j] = fma(av[i], bv[j], acc[i][j]);
          }
          __syncthreads();
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int gi = ti * 64 + ty * 4 + i, gj = tj * 64 + tx * 4 + j;
            if (gi < d && gj < d) {
              const double v = acc[i][j] / (double)n;
              r0[gi * m + gj] = v;
              if (ti != tj) r0[gj * m + gi] = v;
            }
          }
      }
    if (m > d)
      for (int i = tid; i < m; i += kAdaptThreads) {
        r0[i * m + d] = 0.0;
        r0[d * m + i] = 0.0;
      }
    for (int i = tid; i < m * m; i += kAdaptThreads) r1[i] = (i / m == i % m) ? 1.0 : 0.0;
    __syncthreads();

    // ---- 2. C = V diag(lambda) V^T
    const int sw1 = jacobi(r0, m, r1, m, m, sh);
    if (tid < d) sh.lam[tid] = r0[tid * m + tid];
    __syncthreads();
    rank_sort(d, sh);
    if (tid < d) sh.red[tid] = sh.lam[sh.perm[tid]];
    __syncthreads();
    if (tid < d) g.eigval[grp * d + tid] = sh.red[tid];
    if (tid == 0) {
      double trace = 0.0;
      for (int i = 0; i < d; ++i) trace += sh.red[i];
      int r = 0;
      if (sw1 >= 0 && trace > 0.0) {
        const double bar = g.target_energy * trace;
        double cum = 0.0;
        r = d;
        for (int k = 1; k <= d; ++k) {
          cum += sh.red[k - 1];
          if (cum > bar) {
            r = k + 1 < d ? k + 1 : d;
            break;
          }
        }
      }
      sh.r = r;
      sweeps[0] = sw1;
      sweeps[1] = 0;
    }
    __syncthreads();
    const int r = sh.r;
    if (r == 0) {
      if (tid == 0) g.dim[grp] = 0;
      continue;
    }
    const int rp = r + (r & 1);

    // ---- 3. P with its signs
    double* pca = g.pca + grp * (int64_t)d * d;
    if (tid < r) sh.vec[tid] = row_sign(r1 + sh.perm[tid] * m, d);
    __syncthreads();
    for (int idx = tid; idx < r * d; idx += kAdaptThreads) {
      const int i = idx / d, j = idx - i * d;
      pca[idx] = sh.vec[i] * r1[sh.perm[i] * m + j];
    }
    __syncthreads();

    // ---- 4. M = P A^-1 (r0, [r, d]); W' = M M^T (r2), B' = M diag(psi) M^T (r3), both [r, rp]
    for (int idx = tid; idx < r * d; idx += kAdaptThreads) {
      const int i = idx / d, j = idx - i * d;
      double sum = 0.0;
      for (int k = 0; k < d; ++k) sum += pca[i * d + k] * g.ainv[(int64_t)k * d + j];
      r0[idx] = sum;
    }
    __syncthreads();
    for (int idx = tid; idx < r * r; idx += kAdaptThreads) {
      const int i = idx / r, j = idx - i * r;
      if (i > j) continue;
      double w = 0.0, b = 0.0;
      for (int k = 0; k < d; ++k) {
        const double mi = r0[i * d + k], mj = r0[j * d + k];
        w += mi * mj;
        b += mi * g.psi[k] * mj;
      }
      r2[i * rp + j] = w;
      r2[j * rp + i] = w;
      r3[i * rp + j] = b;
      r3[j * rp + i] = b;
    }
    __syncthreads();

    // ---- 5. W' = L L^T in place (the strict lower triangle of r2; the diagonal of L in sh.lam)
    bool spd = true;
    for (int j = 0; j < r; ++j) {
      const double piv = r2[j * rp + j];
      if (!(piv > 0.0)) {
        spd = false;
        break;
      }
      const double l = sqrt(piv);
      if (tid == 0) sh.lam[j] = l;
      for (int i = j + 1 + tid; i < r; i += kAdaptThreads) r2[i * rp + j] /= l;
      __syncthreads();
      const int cnt = r - 1 - j;
      for (int idx = tid; idx < cnt * cnt; idx += kAdaptThreads) {
        const int ii = idx / cnt, kk = idx - ii * cnt;
        if (kk > ii) continue;
        const int i = j + 1 + ii, k = j + 1 + kk;
        r2[i * rp + k] -= r2[i * rp + j] * r2[k * rp + j];
      }
      __syncthreads();
    }
    if (!spd) {
      if (tid == 0) g.dim[grp] = 0;
      continue;
    }

    // ---- 6. L^-1 (r1, [r, rp], lower), one column per thread; K = L^-1 B' L^-T (r3), U^T = I (r2)
    for (int c = tid; c < r; c += kAdaptThreads) {
      for (int i = 0; i < c; ++i) r1[i * rp + c] = 0.0;
      r1[c * rp + c] = 1.0 / sh.lam[c];
      for (int i = c + 1; i < r; ++i) {
        double sum = 0.0;
        for (int k = c; k < i; ++k) sum += r2[i * rp + k] * r1[k * rp + c];
        r1[i * rp + c] = -sum / sh.lam[i];
      }
    }
    __syncthreads();
    for (int idx = tid; idx < r * r; idx += kAdaptThreads) {      // r0 = L^-1 B'
      const int i = idx / r, j = idx - i * r;
      double sum = 0.0;
      for (int k = 0; k <= i; ++k) sum += r1[i * rp + k] * r3[k * rp + j];
      r0[i * rp + j] = sum;
    }
    __syncthreads();
    for (int idx = tid; idx < rp * rp; idx += kAdaptThreads) {
      const int i = idx / rp, j = idx - i * rp;
      r2[idx] = i == j ? 1.0 : 0.0;
      if (i >= r || j >= r) {
        r3[idx] = 0.0;
        continue;
      }
      if (i > j) continue;
      double sum = 0.0;
      for (int k = 0; k <= j; ++k) sum += r0[i * rp + k] * r1[j * rp + k];
      r3[i * rp + j] = sum;
      r3[j * rp + i] = sum;
    }
    __syncthreads();

    // ---- 7. K = U diag(psi') U^T
    const int sw2 = jacobi(r3, rp, r2, rp, rp, sh);
    if (tid == 0) sweeps[1] = sw2;
    if (sw2 < 0) {
      if (tid == 0) g.dim[grp] = 0;
      continue;
    }
    if (tid < r) sh.lam[tid] = r3[tid * rp + tid];
    __syncthreads();
    rank_sort(r, sh);
    if (tid < r) {
      const double v = sh.lam[sh.perm[tid]];
      g.psi_out[grp * d + tid] = v > 0.0 ? v : 0.0;
    }

    // ---- 8. A' = U^T L^-1 (r0, [r, rp]); T = [A' P | -A' P m] with its signs
    for (int idx = tid; idx < r * r; idx += kAdaptThreads) {
      const int i = idx / r, j = idx - i * r;
      const double* u = r2 + sh.perm[i] * rp;
      double sum = 0.0;
      for (int k = j; k < r; ++k) sum += u[k] * r1[k * rp + j];
      r0[i * rp + j] = sum;
    }
    __syncthreads();
    double* aff = g.affine + grp * (int64_t)d * (d + 1);
    for (int idx = tid; idx < r * d; idx += kAdaptThreads) {
      const int i = idx / d, j = idx - i * d;
      double sum = 0.0;
      for (int k = 0; k < r; ++k) sum += r0[i * rp + k] * pca[k * d + j];
      aff[i * (d + 1) + j] = sum;
    }
    __syncthreads();
    if (tid < r) {
      double* row = aff + tid * (d + 1);
      double sum = 0.0;
      for (int j = 0; j < d; ++j) sum += row[j] * g.mean[j];
      row[d] = -sum;
      sh.vec[tid] = row_sign(row, d + 1);
    }
    __syncthreads();
    for (int idx = tid; idx < r * (d + 1); idx += kAdaptThreads)
      if (sh.vec[idx / (d + 1)] < 0.0) aff[idx] = -aff[idx];
    if (tid == 0) g.dim[grp] = r;
  }
}

int64_t adapt_table_bytes(int64_t num_groups) { return (16 * num_groups + 8 + 255) / 256 * 256; }

int64_t adapt_slot_bytes(int d) {
  const int64_t m = d + (d & 1);
  return 4 * m * m * (int64_t)sizeof(double);
}

void free_offsets(void* p) { delete static_cast<std::vector<int64_t>*>(p); }

}  // namespace

int64_t plda_adapt_slot_bytes(int d) { return adapt_slot_bytes(d); }

int64_t plda_adapt_workspace_bytes(int64_t num_groups, int d) { return adapt_table_bytes(num_groups) + adapt_slot_bytes(d); }

hipError_t launch_plda_adapt(const float* x, int64_t ldx, const int64_t* offsets, int64_t num_groups, int d, const double* mean,
                             const double* within_factor, const double* psi, double target_energy, int32_t* dim, double* eigval,
                             double* pca, double* affine, double* psi_out, void* ws, int64_t ws_bytes, hipStream_t stream) {
  const int64_t table = adapt_table_bytes(num_groups), slot = adapt_slot_bytes(d);
  int64_t slots = std::min<int64_t>(std::min<int64_t>((ws_bytes - table) / slot, num_groups), kAdaptMaxSlots);
  if (slots < 1) slots = 1;              // the caller has checked ws_bytes >= table + slot
  auto* copy = new std::vector<int64_t>(offsets, offsets + num_groups + 1);
  hipError_t e = hipMemcpyAsync(ws, copy->data(), copy->size() * sizeof(int64_t), hipMemcpyHostToDevice, stream);
  const int m = d + (d & 1);
  const int use_lds = m <= kAdaptLdsDim;
  if (e == hipSuccess) {
    static std::mutex mu;            // per-device attribute; any thread may make the first launch on a device
    static size_t set_for[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    std::lock_guard<std::mutex> lock(mu);
    if (!set_for[dev & 63]) {
      e = hipFuncSetAttribute(reinterpret_cast<const void*>(plda_adapt_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                              kAdaptLdsDim * kAdaptLdsDim * (int)sizeof(double));
      if (e == hipSuccess) set_for[dev & 63] = 1;
    }
  }
  if (e == hipSuccess) {
    AdaptArgs a;
    a.x = x;
    a.ldx = ldx;
    a.offsets = static_cast<const int64_t*>(ws);
    a.sweeps = reinterpret_cast<int32_t*>(static_cast<char*>(ws) + 8 * (num_groups + 1));
    a.num_groups = num_groups;
    a.d = d;
    a.mean = mean;
    a.ainv = within_factor;
    a.psi = psi;
    a.target_energy = target_energy;
    a.dim = dim;
    a.eigval = eigval;
    a.pca = pca;
    a.affine = affine;
    a.psi_out = psi_out;
    a.slots = reinterpret_cast<double*>(static_cast<char*>(ws) + table);
    a.slot_doubles = slot / (int64_t)sizeof(double);
    a.use_lds = use_lds;
    hipLaunchKernelGGL(plda_adapt_kernel, dim3((unsigned)slots), dim3(kAdaptThreads),
                       use_lds ? (size_t)m * m * sizeof(double) : 0, stream, a);
    e = hipGetLastError();
  }
  // the copy may still be reading the offsets when this returns: they are freed in stream order, behind the copy
  if (hipLaunchHostFunc(stream, free_offsets, copy) != hipSuccess) {
    (void)hipStreamSynchronize(stream);
    delete copy;
  }
  return e;
}

}  // namespace xv
