// The transpose in front of the NT products whose operand is stored the other way round (csrc/nt_gemm.h).
#include "nt_gemm.h"

namespace xv {
namespace ntg {

// dst [cols, ldd] = src [rows, lds]^T, 64 x 64 through LDS; grid (ceil(rows / 64), ceil(cols / 64))
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

hipError_t nt_transpose(const float* src, int64_t lds, int64_t rows, int64_t cols, float* dst, int64_t ldd, hipStream_t s) {
  hipLaunchKernelGGL(nt_transpose_kernel, dim3((unsigned)((rows + 63) / 64), (unsigned)((cols + 63) / 64)), dim3(256), 0, s, src, lds,
                     rows, cols, dst, ldd);
  return hipGetLastError();
}

}  // namespace ntg
}  // namespace xv
