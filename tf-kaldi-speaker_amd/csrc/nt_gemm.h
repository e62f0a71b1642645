// The tile skeleton of the exact-fp32 NT products C = A . B^T shared by csrc/loss_grad.hip and csrc/seg_grad.hip:
// v_mfma_f32_32x32x2_f32, K in steps of 32, [row][32 + 4] floats in LDS, register-staged double buffering, zero-filled
// edges.  A kernel owns its accumulator start and its epilogue; nt_mainloop is everything in between.  The order of the fmaf
// chain of one element is a function of K alone: k ascending in groups of eight, lane half h feeding k = 8 q + 4 h + j.
#pragma once

#include <mutex>

#include "xv_kernels.h"

namespace xv {
namespace ntg {

typedef float gf32x16 __attribute__((ext_vector_type(16)));
typedef float gf32x4 __attribute__((ext_vector_type(4)));

constexpr int GBK = 32;
constexpr int GLDT = GBK + 4;                 // padded LDS row (floats), as csrc/loss.hip

__host__ __device__ constexpr int64_t up(int64_t v, int64_t a) { return (v + a - 1) / a * a; }

template <int BM, int BN>
constexpr size_t nt_smem_bytes() { return (size_t)2 * (BM + BN) * GLDT * sizeof(float); }

// Where element e of lane (r32, h) of the accumulator of wave (wm, wn), sub-tile (ai, bi) lies in C: D[8 * (e / 4) + 4 * h +
// e % 4][r32] (A row, B row).
template <int BM, int BN>
struct NtPos {
  static constexpr int WM = BM / 2, WN = BN / 2;            // per wave
  static constexpr int AI = WM / 32, BI = WN / 32;
  int m0, n0, wm, wn, r32, h;
  __device__ NtPos(int mt, int nt) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    m0 = mt * BM; n0 = nt * BN; wm = wave >> 1; wn = wave & 1; r32 = lane & 31; h = lane >> 5;
  }
  __device__ int row(int ai, int e) const { return m0 + wm * WM + ai * 32 + 8 * (e >> 2) + 4 * h + (e & 3); }
  __device__ int col(int bi) const { return n0 + wn * WN + bi * 32 + r32; }
};

// acc += A [M, K] (rows m0 ..) . B [N, K]^T (rows n0 ..); 256 threads, smem of nt_smem_bytes<BM, BN>().  VEC: both operands
// are 16-byte aligned with leading dimensions that are multiples of 4.
template <int BM, int BN, bool VEC>
__device__ __forceinline__ void nt_mainloop(const float* __restrict__ A, int64_t lda, int M, const float* __restrict__ B, int64_t ldb,
                                            int N, int K, int m0, int n0, gf32x16 (&acc)[BM / 64][BN / 64], float* smem) {
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
  const int c4 = tid & 7, lr = tid >> 3;
  const int nk = (K + GBK - 1) / GBK;

  gf32x4 ra[RA], rb[RB];
  auto load_rows = [&](const float* base, int64_t ld, int row0, int nrows, int kt, gf32x4* r, int passes) {
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
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (k + e < K) v[e] = src[e];
        }
      }
      r[i] = v;
    }
  };
  auto load_tiles = [&](int kt) {
    load_rows(A, lda, m0, M, kt, ra, RA);
    load_rows(B, ldb, n0, N, kt, rb, RB);
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

// Launch `kernel` (one 256-thread workgroup per tile, nt_smem_bytes of dynamic LDS) on `tiles` tiles.  The LDS attribute is
// per device and per kernel: `set_for` and `mu` belong to the instantiation that calls this.
template <class Args>
hipError_t nt_launch(void (*kernel)(Args), size_t smem, std::mutex& mu, bool (&set_for)[64], int64_t tiles, const Args& a,
                     hipStream_t s) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) dev = 0;
  {
    std::lock_guard<std::mutex> lock(mu);
    if (!set_for[dev & 63]) {
      const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                               (int)smem);
      if (e != hipSuccess) return e;
      set_for[dev & 63] = true;
    }
  }
  hipLaunchKernelGGL(kernel, dim3((unsigned)tiles), dim3(256), smem, s, a);
  return hipGetLastError();
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// dst [cols, ldd] = src [rows, lds]^T, 64 x 64 through LDS; grid (ceil(rows / 64), ceil(cols / 64)), cols <= 65535 * 64
static __global__ __launch_bounds__(256) void nt_transpose_kernel(const float* __restrict__ src, int64_t lds, int64_t rows, int64_t cols,
                                                                  float* __restrict__ dst, int64_t ldd) {
  __shared__ float tile[64][65];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t r0 = (int64_t)blockIdx.x * 64, c0 = (int64_t)blockIdx.y * 64;      // rows on x: no 65535 limit
  for (int rl = wave; rl < 64; rl += 4)
    tile[rl][lane] = (r0 + rl < rows && c0 + lane < cols) ? src[(r0 + rl) * lds + c0 + lane] : 0.f;
  __syncthreads();
  for (int cl = wave; cl < 64; cl += 4)
    if (c0 + cl < cols && r0 + lane < rows) dst[(c0 + cl) * ldd + r0 + lane] = tile[lane][cl];
}

inline hipError_t nt_transpose(const float* src, int64_t lds, int64_t rows, int64_t cols, float* dst, int64_t ldd, hipStream_t s) {
  hipLaunchKernelGGL(nt_transpose_kernel, dim3((unsigned)((rows + 63) / 64), (unsigned)((cols + 63) / 64)), dim3(256), 0, s, src, lds,
                     rows, cols, dst, ldd);
  return hipGetLastError();
}

}  // namespace ntg
}  // namespace xv
