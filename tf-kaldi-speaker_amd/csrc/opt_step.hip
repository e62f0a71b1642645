// One optimizer step on one float32 parameter tensor, in place: the TensorFlow 1.x rules the reference trains with
// (model/trainer.py:225-246 optimizers, :529-533 tf.clip_by_norm per tensor, model/loss.py:26-33 the l2 regularizer, whose
// gradient l2 * w is part of total_loss and therefore comes before the clip).  The rule and its operation order are stated in
// include/xvec_hip.h (xv_opt_step); tests/helpers/ref_loss_grad.py writes it in numpy float32 and gets the same bits.
//
// Arithmetic.  Every product, sum, division and square root is rounded to float32 on its own (`#pragma clang fp contract(off)`,
// as csrc/calibrate.hip: hipcc would contract a * b + c into an fma).  Divisions and square roots go through double and are
// rounded back: with 53 >= 2 * 24 + 2 bits the double rounding is innocuous, so the result is the correctly rounded float32
// quotient / root whatever the compiler's fp32 division is.
//
//  * opt_norm_kernel (clip_norm > 0 only): a workgroup of 256 threads owns kOptChunk = 4096 consecutive elements; thread t adds
//    the squares of g_j + l2 w_j (the float32 value the update will use) for j = 256 i + t, i = 0 .. 15, in double, then a
//    shuffle tree (offsets 32 .. 1) and the four waves in wave order: one double per workgroup in the workspace.
//  * opt_update_kernel: every workgroup first adds ALL partials, lane l of wave 0 the partials l, l + 64, ... in ascending order
//    and the same tree (the second fixed-order pass; a few hundred doubles at the sizes of a softmax layer), then updates its
//    elements.  No atomics: the result is a pure function of the inputs.
#include "xv_kernels.h"

namespace xv {

namespace {

constexpr int kOptChunk = 4096;

__device__ __forceinline__ float opt_div(float a, float b) { return (float)((double)a / (double)b); }
__device__ __forceinline__ float opt_sqrt(float a) { return (float)sqrt((double)a); }

__device__ __forceinline__ float opt_grad_l2(float g, float w, float l2) {
#pragma clang fp contract(off)
  if (l2 == 0.f) return g;
  const float p = l2 * w;
  return g + p;
}

__global__ __launch_bounds__(256) void opt_norm_kernel(const float* __restrict__ w, const float* __restrict__ g, int64_t count,
                                                       float l2, double* __restrict__ part) {
#pragma clang fp contract(off)
  __shared__ double red[4];
  const int64_t base = (int64_t)blockIdx.x * kOptChunk;
  double acc = 0.0;
  for (int i = 0; i < kOptChunk / 256; ++i) {
    const int64_t j = base + 256 * i + threadIdx.x;
    if (j < count) {
      const double v = (double)opt_grad_l2(g[j], w[j], l2);
      const double sq = v * v;
      acc = acc + sq;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

struct OptArgs {
  int kind, nesterov;
  float lr, l2, clip, mom, b1, b2, omb1, omb2, eps;     // lr: lr_t for adam
};

__global__ __launch_bounds__(256) void opt_update_kernel(float* __restrict__ w, const float* __restrict__ g, float* __restrict__ s0,
                                                         float* __restrict__ s1, int64_t count, OptArgs p,
                                                         const double* __restrict__ part, int64_t nparts) {
#pragma clang fp contract(off)
  __shared__ float denom_s;
  float denom = 0.f;
  if (p.clip > 0.f) {
    if (threadIdx.x < 64) {
      double v = 0.0;
      for (int64_t c = threadIdx.x; c < nparts; c += 64) v += part[c];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
      if (threadIdx.x == 0) {
        const float nrm = (float)sqrt(v);
        denom_s = nrm > p.clip ? nrm : p.clip;               // max(||g||, clip_norm)
      }
    }
    __syncthreads();
    denom = denom_s;
  }
  const int64_t base = (int64_t)blockIdx.x * kOptChunk;
  for (int i = 0; i < kOptChunk / 256; ++i) {
    const int64_t j = base + 256 * i + threadIdx.x;
    if (j >= count) break;
    float wj = w[j];
    float gj = opt_grad_l2(g[j], wj, p.l2);
    if (p.clip > 0.f) {
      const float t = gj * p.clip;
      gj = opt_div(t, denom);
    }
    if (p.kind == XV_OPT_SGD) {
      const float d = p.lr * gj;
      wj = wj - d;
    } else if (p.kind == XV_OPT_MOMENTUM) {
      const float ma = p.mom * s0[j];
      const float a = ma + gj;
      s0[j] = a;
      if (p.nesterov) {
        const float ma2 = p.mom * a;
        const float t = gj + ma2;
        const float d = p.lr * t;
        wj = wj - d;
      } else {
        const float d = p.lr * a;
        wj = wj - d;
      }
    } else {
      const float m1 = p.b1 * s0[j];
      const float m2 = p.omb1 * gj;
      const float m = m1 + m2;
      const float gg = gj * gj;
      const float v1 = p.b2 * s1[j];
      const float v2 = p.omb2 * gg;
      const float v = v1 + v2;
      s0[j] = m;
      s1[j] = v;
      const float num = p.lr * m;
      const float den = opt_sqrt(v) + p.eps;
      wj = wj - opt_div(num, den);
    }
    w[j] = wj;
  }
}

}  // namespace

int64_t opt_workspace_bytes(int64_t count) { return count > 0 ? (count + kOptChunk - 1) / kOptChunk * 8 : 0; }

hipError_t launch_opt_step(int kind, int nesterov, float* w, const float* g, float* slot0, float* slot1, int64_t count, double lr,
                           double l2, double clip_norm, double momentum, int64_t step, void* ws, hipStream_t s) {
  if (count <= 0) return hipSuccess;
  OptArgs p = {};
  p.kind = kind;
  p.nesterov = nesterov;
  p.l2 = (float)l2;
  p.clip = (float)clip_norm;
  p.mom = (float)momentum;
  p.b1 = 0.9f;
  p.b2 = 0.999f;
  p.omb1 = (float)(1.0 - 0.9);
  p.omb2 = (float)(1.0 - 0.999);
  p.eps = 1e-8f;
  p.lr = (float)lr;
  if (kind == XV_OPT_ADAM) p.lr = (float)(lr * sqrt(1.0 - pow(0.999, (double)step)) / (1.0 - pow(0.9, (double)step)));
  const int64_t nparts = (count + kOptChunk - 1) / kOptChunk;
  double* part = static_cast<double*>(ws);
  if (p.clip > 0.f) {
    hipLaunchKernelGGL(opt_norm_kernel, dim3((unsigned)nparts), dim3(256), 0, s, w, g, count, p.l2, part);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(opt_update_kernel, dim3((unsigned)nparts), dim3(256), 0, s, w, g, slot0, slot1, count, p, part, nparts);
  return hipGetLastError();
}

}  // namespace xv
