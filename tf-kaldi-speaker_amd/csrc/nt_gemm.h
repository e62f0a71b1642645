// The one exact-fp32 tile product C = A . B^T of the library: v_mfma_f32_32x32x2_f32, K in steps of 32, [row][32 + 4] floats in
// LDS (conflict-free ds_read_b128), register-staged double buffering, edges of M, N and K zero-filled by the loaders (nothing is
// pre-packed).  Users: score_tile_kernel (csrc/score.hip) and loss_tile_kernel (csrc/loss.hip), persistent 128 x 128 kernels that
// walk their tiles by nt_tile; nt_gemm_kernel (csrc/loss_grad.hip) and seg_gemm_kernel (csrc/seg_grad.hip), one tile per
// workgroup.  csrc/tconv_grad.hip shares NtPos only: its gathered, partly K-major operand tiles are a different loop.
//
// A kernel owns its argument struct, what it stages in LDS behind the operand tiles, its accumulator start (zero, or
// nt_acc_start), its epilogue (positions by NtPos) and the barrier after an epilogue that reuses LDS; nt_mainloop is everything
// in between and ends on a barrier, so the operand tiles are dead when it returns.  nt_launch sets the LDS attribute.
//
// The order of the fmaf chain of one element is a function of K alone: k ascending in groups of eight, lane half h feeding
// k = 8 q + 4 h + j; the MFMAs of a group are issued by j, then ai, then bi, so every accumulator takes its k in ascending j.
#pragma once

#include <mutex>

#include "wave_reduce.h"
#include "xv_kernels.h"

namespace xv {
namespace ntg {

typedef float gf32x16 __attribute__((ext_vector_type(16)));
typedef float gf32x4 __attribute__((ext_vector_type(4)));

constexpr int GBK = 32;
constexpr int GLDT = GBK + 4;                 // padded LDS row (floats)
constexpr int GGROUP = 8;                     // tile rows per group of nt_tile

__host__ __device__ constexpr int64_t up(int64_t v, int64_t a) { return (v + a - 1) / a * a; }

template <int BM, int BN>
constexpr size_t nt_smem_bytes() { return (size_t)2 * (BM + BN) * GLDT * sizeof(float); }

// Where element e of lane (r32, h) of the accumulator of wave (wm, wn), sub-tile (ai, bi) lies in C: D[8 * (e / 4) + 4 * h +
// e % 4][r32] (A row, B row).  lrow / lcol count from the tile's corner.
template <int BM, int BN>
struct NtPos {
  static constexpr int WM = BM / 2, WN = BN / 2;            // per wave
  static constexpr int AI = WM / 32, BI = WN / 32;
  int m0, n0, wm, wn, r32, h;
  __device__ NtPos(int mt, int nt) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    m0 = mt * BM; n0 = nt * BN; wm = wave >> 1; wn = wave & 1; r32 = lane & 31; h = lane >> 5;
  }
  __device__ int lrow(int ai, int e) const { return wm * WM + ai * 32 + 8 * (e >> 2) + 4 * h + (e & 3); }
  __device__ int lcol(int bi) const { return wn * WN + bi * 32 + r32; }
  __device__ int row(int ai, int e) const { return m0 + lrow(ai, e); }
  __device__ int col(int bi) const { return n0 + lcol(bi); }
};

// Tile t of an nMt x nNt grid in the order of the persistent kernels: groups of GGROUP tile rows, walked column by column, so
// that the workgroups in flight share 8 A panels and ~64 B panels.
__device__ __forceinline__ void nt_tile(int64_t t, int nMt, int nNt, int& mt, int& nt) {
  const int64_t per_group = (int64_t)GGROUP * nNt;
  const int g = (int)(t / per_group);
  const int gm = min(GGROUP, nMt - g * GGROUP);
  const int64_t tg = t - g * per_group;
  nt = (int)(tg / gm);
  mt = g * GGROUP + (int)(tg - (int64_t)nt * gm);
}

// acc = 0, or (`resume`) out [M, N] at the tile: the chain goes on from where an earlier launch left it
template <int BM, int BN>
__device__ __forceinline__ void nt_acc_start(gf32x16 (&acc)[BM / 64][BN / 64], const NtPos<BM, BN>& at, bool resume = false,
                                             const float* out = nullptr, int64_t ldo = 0, int M = 0, int N = 0) {
#pragma unroll
  for (int ai = 0; ai < BM / 64; ++ai)
#pragma unroll
    for (int bi = 0; bi < BN / 64; ++bi)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        float v = 0.f;
        if (resume) {
          const int gi = at.row(ai, e), gj = at.col(bi);
          if (gi < M && gj < N) v = out[(int64_t)gi * ldo + gj];
        }
        acc[ai][bi][e] = v;
      }
}

// acc += A [M, K] (rows m0 ..) . B [N, K]^T (rows n0 ..); 256 threads, smem of nt_smem_bytes<BM, BN>().  VEC: both operands
// are 16-byte aligned with leading dimensions that are multiples of 4.  SUB: a_sub [K] (if not null) is subtracted from every
// A row while it is staged.
template <int BM, int BN, bool VEC, bool SUB = false>
__device__ __forceinline__ void nt_mainloop(const float* __restrict__ A, int64_t lda, int M, const float* __restrict__ B, int64_t ldb,
                                            int N, int K, int m0, int n0, gf32x16 (&acc)[BM / 64][BN / 64], float* smem,
                                            const float* a_sub = nullptr) {
  constexpr int TA = BM * GLDT, TB = BN * GLDT;      // floats per operand tile
  constexpr int WM = BM / 2, WN = BN / 2;
  constexpr int AI = WM / 32, BI = WN / 32;
  constexpr int RA = BM / 32, RB = BN / 32;          // staging passes
  float* As = smem;                    // [2][BM][GLDT]
  float* Bs = smem + 2 * TA;           // [2][BN][GLDT]

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int r32 = lane & 31, h = lane >> 5;
  const int c4 = tid & 7, lr = tid >> 3;             // staging map: thread -> (row lr + 32 * i, float4 column c4)
  const int nk = (K + GBK - 1) / GBK;

  gf32x4 ra[RA], rb[RB];
  auto load_rows = [&](const float* base, int64_t ld, int row0, int nrows, int kt, gf32x4* r, int passes, const float* sub) {
    const int k = kt * GBK + c4 * 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (i >= passes) break;
      const int row = row0 + lr + 32 * i;
      gf32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (row < nrows && k < K) {
        const float* src = base + (int64_t)row * ld + k;
        if (VEC && k + 4 <= K) {
          v = *reinterpret_cast<const gf32x4*>(src);
          if (SUB && sub) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] -= sub[k + e];
          }
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (k + e < K) v[e] = (SUB && sub) ? src[e] - sub[k + e] : src[e];
        }
      }
      r[i] = v;
    }
  };
  auto load_tiles = [&](int kt) {
    load_rows(A, lda, m0, M, kt, ra, RA, a_sub);
    load_rows(B, ldb, n0, N, kt, rb, RB, nullptr);
  };
  auto store_tiles = [&](int buf) {
#pragma unroll
    for (int i = 0; i < RA; ++i) *reinterpret_cast<gf32x4*>(As + buf * TA + (lr + 32 * i) * GLDT + c4 * 4) = ra[i];
#pragma unroll
    for (int i = 0; i < RB; ++i) *reinterpret_cast<gf32x4*>(Bs + buf * TB + (lr + 32 * i) * GLDT + c4 * 4) = rb[i];
  };

  load_tiles(0);
  store_tiles(0);
  __syncthreads();

  const float* a_base = As + (wm * WM + r32) * GLDT + 4 * h;
  const float* b_base = Bs + (wn * WN + r32) * GLDT + 4 * h;
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < nk) load_tiles(kt + 1);
    const float* ap = a_base + cur * TA;
    const float* bp = b_base + cur * TB;
#pragma unroll
    for (int q = 0; q < GBK / 8; ++q) {
      // lane (r, h) feeds k = 8 q + 4 h + j of both operands: the order of the chain is a function of k alone
      gf32x4 a[AI], b[BI];
#pragma unroll
      for (int ai = 0; ai < AI; ++ai) a[ai] = *reinterpret_cast<const gf32x4*>(ap + ai * 32 * GLDT + q * 8);
#pragma unroll
      for (int bi = 0; bi < BI; ++bi) b[bi] = *reinterpret_cast<const gf32x4*>(bp + bi * 32 * GLDT + q * 8);
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int ai = 0; ai < AI; ++ai)
#pragma unroll
          for (int bi = 0; bi < BI; ++bi)
            acc[ai][bi] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[ai][j], b[bi][j], acc[ai][bi], 0, 0, 0);
    }
    if (kt + 1 < nk) store_tiles(cur ^ 1);
    __syncthreads();
  }
}

// Launch KERNEL with `grid` 256-thread workgroups and `smem` bytes of dynamic LDS.  The LDS attribute is per device and per
// kernel, and any thread may make the first launch on a device: it is raised whenever a call asks for more than the device
// has been given so far.
template <auto KERNEL, class Args>
hipError_t nt_launch(size_t smem, int64_t grid, const Args& a, hipStream_t s) {
  static std::mutex mu;
  static size_t set_for[64] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) dev = 0;
  {
    std::lock_guard<std::mutex> lock(mu);
    if (set_for[dev & 63] < smem) {
      const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize,
                                               (int)smem);
      if (e != hipSuccess) return e;
      set_for[dev & 63] = smem;
    }
  }
  hipLaunchKernelGGL(KERNEL, dim3((unsigned)grid), dim3(256), smem, s, a);
  return hipGetLastError();
}

// the operands of a product allow VEC
inline bool nt_vec(const float* a, int64_t lda, const float* b, int64_t ldb) {
  return aligned16(a) && aligned16(b) && lda % 4 == 0 && ldb % 4 == 0;
}

// dst [cols, ldd] = src [rows, lds]^T (csrc/nt_transpose.hip); cols <= 65535 * 64
hipError_t nt_transpose(const float* src, int64_t lds, int64_t rows, int64_t cols, float* dst, int64_t ldd, hipStream_t s);

}  // namespace ntg
}  // namespace xv
